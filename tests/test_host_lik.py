"""CPU tests of the torch route of the scalar non-Gaussian likelihoods (vidp_amd.likelihoods.Bernoulli / Poisson /
ScalarQuadratureLikelihood) against the NumPy restatement tests/np_lik.py and against the identities of the contract."""
import math

import numpy as np
import pytest

from tests import np_lik


@pytest.fixture(scope="module")
def L():
    import vidp_amd  # noqa: F401
    from vidp_amd import likelihoods
    return likelihoods


def T(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))


def draws(rng, n, vmax=1e2):
    mu = rng.uniform(-8, 8, size=(n, 1))
    var = 10.0 ** rng.uniform(-6, np.log10(vmax), size=(n, 1))
    return mu, var


def test_bernoulli_torch_route_matches_numpy(L, rng):
    mu, var = draws(rng, 4000)
    y = rng.integers(0, 2, size=(4000, 1)).astype(np.float64)
    lik, ref = L.Bernoulli(), np_lik.Bernoulli()
    ve, dmu, dv, sc = ref.ve_and_grads(mu, var, y)
    got = lik.variational_expectations(T(mu), T(var), T(y)).numpy()
    assert got.shape == (4000,)
    np.testing.assert_allclose(got, ve[:, 0], rtol=0, atol=1e-12 * sc["ve"].max())
    assert np.all(np.abs(got - ve[:, 0]) <= 1e-12 * sc["ve"][:, 0])
    g1, g2 = (x.numpy() for x in lik.ve_gradients_expectation(T(mu), T(var), T(y)))
    assert g1.shape == g2.shape == (4000, 1)
    assert np.all(np.abs(g2 - dv) <= 1e-12 * sc["dv"])
    assert np.all(np.abs(g1 - (dmu - 2 * dv * mu)) <= 1e-12 * (sc["dmu"] + 2 * np.abs(mu) * sc["dv"]))


def test_poisson_torch_route_matches_numpy(L, rng):
    mu = rng.uniform(-4, 3, size=(3000, 1))
    var = 10.0 ** rng.uniform(-6, 0.5, size=(3000, 1))
    y = rng.poisson(3.0, size=(3000, 1)).astype(np.float64)
    for b in (1.0, 0.3):
        lik, ref = L.Poisson(b), np_lik.Poisson(b)
        ve, dmu, dv, sc = ref.ve_and_grads(mu, var, y)
        got = lik.variational_expectations(T(mu), T(var), T(y)).numpy()
        assert np.all(np.abs(got - ve[:, 0]) <= 1e-12 * sc["ve"][:, 0])
        g1, g2 = (x.numpy() for x in lik.ve_gradients_expectation(T(mu), T(var), T(y)))
        np.testing.assert_allclose(g2, dv, rtol=1e-12)
        assert np.all(np.abs(g1 - (dmu - 2 * dv * mu)) <= 1e-12 * (sc["dmu"] + 2 * np.abs(mu) * sc["dv"]))


def test_autograd_gradients_equal_the_formulas(L, rng):
    """The torch route's gradients come from autograd through the rule; the formulas of the contract written out in torch."""
    import torch
    mu, var = draws(rng, 500, vmax=10.0)
    y = rng.integers(0, 2, size=(500, 1)).astype(np.float64)
    lik = L.Bernoulli()
    g1, g2 = lik.ve_gradients_expectation(T(mu), T(var), T(y))
    j, c = 1e-3, 1 - 2e-3
    xi = torch.tensor(np_lik.XI, dtype=torch.float64)
    W = torch.tensor(np_lik.W, dtype=torch.float64)
    X = T(mu) + math.sqrt(2) * torch.sqrt(T(var)) * xi
    s = torch.where(T(y) == 1, 1.0, -1.0).double()
    dl = s * c * torch.exp(-0.5 * X * X) / math.sqrt(2 * math.pi) / (j + c * 0.5 * torch.erfc(-s * X / math.sqrt(2)))
    dmu = (W * dl).sum(-1, keepdim=True)
    dv = (W * dl * xi).sum(-1, keepdim=True) / (math.sqrt(2) * torch.sqrt(T(var)))
    scale_v = (W * (dl * xi).abs()).sum(-1, keepdim=True) / (math.sqrt(2) * torch.sqrt(T(var)))
    assert bool(((g2 - dv).abs() <= 1e-12 * scale_v).all())
    assert bool(((g1 - (dmu - 2 * dv * T(mu))).abs() <= 1e-12 * ((W * dl.abs()).sum(-1, keepdim=True) + 2 * T(mu).abs() * scale_v)).all())
    # Poisson: dmu = y - m, dv = -m / 2
    yp = rng.poisson(2.0, size=(500, 1)).astype(np.float64)
    mu2 = rng.uniform(-3, 2, size=(500, 1))
    g1, g2 = (x.numpy() for x in L.Poisson(2.0).ve_gradients_expectation(T(mu2), T(var), T(yp)))
    m = 2.0 * np.exp(mu2 + 0.5 * var)
    np.testing.assert_allclose(g2, -0.5 * m, rtol=1e-13)
    np.testing.assert_allclose(g1, yp - m + m * mu2, rtol=1e-12, atol=1e-12 * (yp + m + m * np.abs(mu2)).max())


def test_bernoulli_probit_identity(L, rng):
    """sum_k W_k p_j(X_k) = p_j(mu / sqrt(1 + v)): exact for the integral, so for the 20-point rule only while the integrand is smooth on
    the rule's scale -- ~1e-15 at v <= 0.1, ~1e-10 at v = 1 (and 1e-4 at v = 4, not asserted)."""
    lik = L.Bernoulli()
    mu = rng.uniform(-5, 5, size=(2000, 1))
    for vmax, tol in ((0.1, 1e-14), (1.0, 1e-9)):
        var = rng.uniform(1e-8, vmax, size=(2000, 1))
        X, W = lik._nodes(T(mu), T(var))
        rule = (lik._p(X) * W).sum(-1).numpy()
        p, pv = (x.numpy() for x in lik.predict_mean_and_var(T(mu), T(var)))
        np.testing.assert_allclose(rule, p, rtol=tol)
        np.testing.assert_allclose(pv, p - p * p, rtol=1e-15)


def test_poisson_closed_form_matches_the_generic_rule(L, rng):
    """For e^f the 20-point Gauss-Hermite remainder is sqrt(pi) 20! / (2^20 40!) (sqrt(2) sigma)^40 e^{...}: below 1e-28 of the exponential
    term at v <= 1, so the closed form and the rule on the same log_prob agree to rounding (1e-13 of the sum of absolute terms)."""
    lik = L.Poisson(0.7)
    generic = L.ScalarQuadratureLikelihood(lik.log_prob)
    assert generic.kind is None
    mu = rng.uniform(-3, 3, size=(2000, 1))
    var = rng.uniform(1e-6, 1.0, size=(2000, 1))
    y = rng.poisson(4.0, size=(2000, 1)).astype(np.float64)
    a = lik.variational_expectations(T(mu), T(var), T(y)).numpy()
    b = generic.variational_expectations(T(mu), T(var), T(y)).numpy()
    sc = np_lik.Poisson(0.7).ve_and_grads(mu, var, y)[3]["ve"][:, 0]
    assert np.all(np.abs(a - b) <= 1e-13 * sc)
    ga, gb = lik.ve_gradients_expectation(T(mu), T(var), T(y)), generic.ve_gradients_expectation(T(mu), T(var), T(y))
    m = 0.7 * np.exp(mu + 0.5 * var)
    assert np.all(np.abs(ga[1].numpy() - gb[1].numpy()) <= 1e-13 * m)
    assert np.all(np.abs(ga[0].numpy() - gb[0].numpy()) <= 1e-13 * (y + m + 2 * m * np.abs(mu)))


@pytest.mark.parametrize("which", ["bernoulli", "poisson"])
def test_central_differences_of_the_rule(L, rng, which):
    """dVE/dmu and dVE/dv are the derivatives of the 20-point rule itself (what a tape over it gives)."""
    import torch
    lik = L.Bernoulli() if which == "bernoulli" else L.Poisson(1.5)
    mu = rng.uniform(-2, 2, size=(50, 1))
    var = rng.uniform(0.05, 2.0, size=(50, 1))
    y = (rng.integers(0, 2, size=(50, 1)) if which == "bernoulli" else rng.poisson(2.0, size=(50, 1))).astype(np.float64)
    g1, g2 = (x.numpy() for x in lik.ve_gradients_expectation(T(mu), T(var), T(y)))
    dv = g2
    dmu = g1 + 2 * dv * mu
    ve = lambda m, v: lik.variational_expectations(T(m), T(v), T(y)).numpy()[:, None]
    h = 1e-4
    fd_mu = (8 * (ve(mu + h / 2, var) - ve(mu - h / 2, var)) - (ve(mu + h, var) - ve(mu - h, var))) / (6 * h)
    fd_v = (8 * (ve(mu, var + h / 2) - ve(mu, var - h / 2)) - (ve(mu, var + h) - ve(mu, var - h))) / (6 * h)
    np.testing.assert_allclose(dmu, fd_mu, rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(dv, fd_v, rtol=1e-7, atol=1e-9)
    assert torch.is_tensor(lik.variational_expectations_sum(T(mu), T(var), T(y)))


def test_bernoulli_labels_other_than_one_count_as_zero(L, rng):
    lik = L.Bernoulli()
    mu, var = draws(rng, 200, vmax=10.0)
    zero = np.zeros((200, 1))
    base = lik.variational_expectations(T(mu), T(var), T(zero)).numpy()
    gb = [x.numpy() for x in lik.ve_gradients_expectation(T(mu), T(var), T(zero))]
    for other in (-1.0, 2.0, 0.5, 0.999):
        y = np.full((200, 1), other)
        np.testing.assert_array_equal(lik.variational_expectations(T(mu), T(var), T(y)).numpy(), base)
        for a, b in zip(lik.ve_gradients_expectation(T(mu), T(var), T(y)), gb):
            np.testing.assert_array_equal(a.numpy(), b)
        np.testing.assert_array_equal(lik.predict_log_density(T(mu), T(var), T(y)).numpy(),
                                      lik.predict_log_density(T(mu), T(var), T(zero)).numpy())


def test_predictions_match_numpy(L, rng):
    mu, var = draws(rng, 300, vmax=10.0)
    y = rng.integers(0, 2, size=(300, 1)).astype(np.float64)
    lik, ref = L.Bernoulli(), np_lik.Bernoulli()
    for a, b in zip(lik.predict_mean_and_var(T(mu), T(var)), ref.predict_mean_and_var(mu, var)):
        np.testing.assert_allclose(a.numpy(), b, rtol=1e-13)
    np.testing.assert_allclose(lik.predict_log_density(T(mu), T(var), T(y)).numpy(), ref.predict_log_density(mu, var, y), rtol=1e-13)
    mu = rng.uniform(-3, 2, size=(300, 1))
    yp = rng.poisson(2.0, size=(300, 1)).astype(np.float64)
    lik, ref = L.Poisson(0.5), np_lik.Poisson(0.5)
    for a, b in zip(lik.predict_mean_and_var(T(mu), T(var)), ref.predict_mean_and_var(mu, var)):
        np.testing.assert_allclose(a.numpy(), b, rtol=1e-13)
    np.testing.assert_allclose(lik.predict_log_density(T(mu), T(var), T(yp)).numpy(), ref.predict_log_density(mu, var, yp), rtol=1e-12)


def test_nonpositive_variance_is_not_clamped(L):
    for lik in (L.Bernoulli(), L.ScalarQuadratureLikelihood(L.Poisson().log_prob)):
        out = lik.variational_expectations(T([[0.3]]), T([[-1e-3]]), T([[1.0]])).numpy()
        assert np.isnan(out).all()


def test_torch_route_is_differentiable(L, rng):
    """classic_elbo_tape / ssm_natgrad run autograd through variational_expectations: gradients flow to the inputs."""
    import torch
    mu = T(rng.uniform(-1, 1, size=(20, 1))).requires_grad_(True)
    var = T(rng.uniform(0.1, 1, size=(20, 1))).requires_grad_(True)
    y = T(rng.integers(0, 2, size=(20, 1)).astype(np.float64))
    lik = L.Bernoulli()
    gm, gv = torch.autograd.grad(lik.variational_expectations(mu, var, y).sum(), [mu, var])
    g1, g2 = lik.ve_gradients_expectation(mu.detach(), var.detach(), y)
    np.testing.assert_allclose(gv.numpy(), g2.numpy(), rtol=1e-14)
    np.testing.assert_allclose(gm.numpy(), (g1 + 2 * g2 * mu.detach()).numpy(), rtol=1e-12, atol=1e-14)
