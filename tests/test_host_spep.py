"""
CPU tests of sparse Power Expectation Propagation: the torch route of vidp_amd.sparse_pep on CPU tensors and the dense NumPy model
tests/np_spep.py against the closed-form fixed-point energy of a Gaussian likelihood, against each other over damped steps, the
pair-normaliser identity against dense chain normalisers, the reference's three tests, improper cavities and argument validation.  No GPU.
"""
import numpy as np
import pytest

from oracle import np_conditionals, np_kernels, np_models
from tests import np_lik, np_pep, np_spep

KINDS = {"gaussian": 0.6, "bernoulli": 1e-3, "poisson": 1.3}


def _kernels(name, scale=1.0):
    from vidp_amd import kernels as K
    mk = {"m12": lambda mod: mod.Matern12(2.0, 2.25 * scale), "m32": lambda mod: mod.Matern32(1.1, 1.2 * scale),
          "m52": lambda mod: mod.Matern52(1.0, 1.5 * scale)}[name]
    return mk(K), mk(np_kernels)


def _lik(kind):
    from vidp_amd.likelihoods import Bernoulli, Gaussian, PEPGaussian, PEPScalarLikelihood, Poisson
    return {"gaussian": lambda: PEPGaussian(Gaussian(KINDS["gaussian"])), "bernoulli": lambda: PEPScalarLikelihood(Bernoulli(1e-3)),
            "poisson": lambda: PEPScalarLikelihood(Poisson(1.3))}[kind]()


def _ve(kind):
    return {"gaussian": np_models.GaussianLik(KINDS["gaussian"]), "bernoulli": np_lik.Bernoulli(1e-3),
            "poisson": np_lik.Poisson(1.3)}[kind].variational_expectations


def _models(kind, kname, z, alpha, lr, scale=1.0):
    import torch
    import vidp_amd  # noqa: F401
    from vidp_amd.sparse_pep import SparsePowerExpectationPropagation
    kt, kn = _kernels(kname, scale)
    g = SparsePowerExpectationPropagation(kt, torch.from_numpy(z), _lik(kind), learning_rate=lr, alpha=alpha)
    o = np_spep.SparsePowerExpectationPropagation(kn, z, kind, KINDS[kind], learning_rate=lr, alpha=alpha, ve=_ve(kind))
    return g, o


def _T(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


@pytest.mark.parametrize("alpha", [1.0, 0.5, 0.1])
@pytest.mark.parametrize("kname", ["m32", "m52"])
def test_closed_form_gaussian_energy(rng, kname, alpha):
    """Gaussian likelihood, M = 30 inducing points 0.25 lengthscales apart, one data point strictly inside every interval (the two
    open end intervals included), so c_i > 0: the converged energy of the torch route and of the dense NumPy model equals
    log N(y; 0, W K_uu W^T + diag(alpha c + s^2)) - (1 - alpha) / (2 alpha) sum_i log(1 + alpha c_i / s^2) to rtol 1e-9 (measured
    here: <= 3e-13 for both models).  alpha = 1 converges in one lr = 1 step; otherwise a step contracts the error by 1 - alpha."""
    ls = 1.1 if kname == "m32" else 1.0
    M = 30
    z = 0.25 * ls * np.arange(M)
    t = np.concatenate([[z[0] - 0.1], 0.5 * (z[1:] + z[:-1]) + 0.03 * rng.uniform(-1, 1, M - 1), [z[-1] + 0.1]])
    y = np.sin(t) + 0.3 * rng.normal(size=t.size)
    g, o = _models("gaussian", kname, z, alpha, 1.0)
    data = (_T(t), _T(y[:, None]))
    for _ in range(1 if alpha == 1.0 else 400):
        old = g.nat2.clone()
        g.update_sites(data)
        o.update_sites(t, y)
        if float((g.nat2 - old).abs().max()) < 1e-14 * float(old.abs().max()):
            break
    g.update_sites(data)
    o.update_sites(t, y)
    seg, w, c = np_spep.data_terms(o.kernel, z, t)
    d = o.d
    W = np.zeros((t.size, (M + 2) * d))
    for i in range(t.size):
        W[i, i * d:(i + 2) * d] = w[i]
    want = np_spep.gaussian_closed_form(np.linalg.inv(o.Pp), W[:, d:-d], c, y, KINDS["gaussian"], alpha)
    assert np.all(c > 0) and g.num_skipped == 0 and o.skipped == 0
    print("closed form residuals", abs(o.energy(t, y) - want), abs(float(g.energy(data)) - want))
    np.testing.assert_allclose(o.energy(t, y), want, rtol=1e-9)
    np.testing.assert_allclose(float(g.energy(data)), want, rtol=1e-9)


def _ragged_data(rng, kind, z):
    """Several points per interval, two empty intervals, points before the first and after the last inducing point."""
    t = np.sort(rng.uniform(z[0] - 0.7, z[-1] + 0.8, size=40))
    t = t[~((t > z[3]) & (t < z[4])) & ~((t > z[7]) & (t < z[8]))]
    f = 1.5 * np.sin(0.6 * t)
    if kind == "gaussian":
        y = f + np.sqrt(KINDS["gaussian"]) * rng.normal(size=t.size)
    elif kind == "bernoulli":
        y = (f + 0.5 * rng.normal(size=t.size) > 0).astype(np.float64)
    else:
        y = rng.poisson(np.exp(0.5 * f)).astype(np.float64)
    return t, y


@pytest.mark.parametrize("alpha", [0.5, 1.0])
@pytest.mark.parametrize("kind", ["gaussian", "bernoulli", "poisson"])
def test_torch_route_against_numpy_model(rng, kind, alpha):
    """The torch route on CPU tensors follows the dense NumPy model over 10 damped steps (lr = 0.5, Matern-3/2, 13 inducing points;
    Poisson at a quarter of the prior variance): sites, log_norm, classic_elbo and energy to 1e-9; nothing is skipped."""
    z = np.linspace(0.0, 6.0, 13)
    t, y = _ragged_data(rng, kind, z)
    g, o = _models(kind, "m32", z, alpha, 0.5, 0.25 if kind == "poisson" else 1.0)
    data = (_T(t), _T(y[:, None]))
    cnt = g.compute_num_data_per_interval(data[0]).numpy()
    assert cnt[0] > 0 and cnt[-1] > 0 and (cnt == 0).sum() >= 2 and cnt.max() >= 3
    for _ in range(10):
        g.update_sites(data)
        o.update_sites(t, y)
        for a, b in ((g.nat1, o.nat1), (g.nat2, o.nat2), (g.log_norm[:, 0], o.log_norm)):
            np.testing.assert_allclose(a.numpy(), b, rtol=1e-9, atol=1e-9 * np.abs(b).max())
        np.testing.assert_allclose(float(g.classic_elbo(data)), o.classic_elbo(t, y), rtol=1e-9)
        np.testing.assert_allclose(float(g.energy(data)), o.energy(t, y), rtol=1e-9)
    assert g.num_skipped == 0 and o.skipped == 0
    np.testing.assert_allclose(g.compute_log_norm(data).numpy(), o.compute_log_norm(t, y), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(g.compute_fraction(data[0]).numpy(), 1.0 / cnt[np.searchsorted(z, t)])


def test_pair_normaliser_identity(rng):
    """The pair form g_c - g_q that the update uses, against the reference's route of two dense chain normalisers: the energy terms
    e_m of np_spep.interval_update and of the torch route's interval_update (energy mode), minus the tilted normalisers log Z_i taken
    at cavities that come from the dense chain with the fraction beta of site m removed, equal n_m (G(chain cavity) - G(chain q)).
    The padded halves of the end sites are zeroed, since the chain does not contain them."""
    import vidp_amd  # noqa: F401
    from vidp_amd.sparse_pep import interval_update
    z = np.linspace(0.0, 3.0, 7)
    t, y = np.sort(rng.uniform(-0.4, 3.5, 15)), rng.normal(size=15)
    o = np_spep.SparsePowerExpectationPropagation(np_kernels.Matern32(1.1, 1.2), z, "gaussian", 0.6, learning_rate=0.7, alpha=0.8)
    o.update_sites(t, y)
    o.update_sites(t, y)
    d = o.d
    o.nat1[0, :d], o.nat2[0, :d, :], o.nat2[0, :, :d] = 0.0, 0.0, 0.0
    o.nat1[-1, d:], o.nat2[-1, d:, :], o.nat2[-1, :, d:] = 0.0, 0.0, 0.0
    seg, w, c = np_spep.data_terms(o.kernel, z, t)
    cnt = np.diff(seg)
    idx = np.repeat(np.arange(len(cnt)), cnt)
    mu, S = o.pair_marginals()
    e_np = np_spep.interval_update("gaussian", seg, w, c, y, mu, S, o.nat1, o.nat2, o.log_norm, 0.6, o.alpha, 0.0)[3]
    e_torch = interval_update(_lik("gaussian"), o.alpha, 0.0, _T(idx).long(), _T(w), _T(c), _T(y), _T(mu), _T(S), _T(o.nat1), _T(o.nat2),
                              _T(o.log_norm))[3].numpy()
    P, mq, _ = o.posterior()
    nq = np_pep.normalizer(P, mq)
    for m in np.nonzero(cnt)[0]:
        beta = o.alpha / cnt[m]
        n1, n2 = o.nat1.copy(), o.nat2.copy()
        n1[m] *= 1 - beta
        n2[m] *= 1 - beta
        Pc, mc, _ = o.posterior(n1, n2)
        cmu, cS = o.pair_marginals(n1, n2)
        i = np.arange(seg[m], seg[m + 1])
        fm, fv = w[i] @ cmu[m], np.einsum("pi,ij,pj->p", w[i], cS[m], w[i]) + c[i]
        lz = np_pep.tilted("gaussian", fm, fv, y[i], 0.6, o.alpha)[0]
        want = cnt[m] * (np_pep.normalizer(Pc, mc) - nq)
        np.testing.assert_allclose(e_np[m] - lz.sum(), want, rtol=1e-9, atol=1e-10)
        np.testing.assert_allclose(e_torch[m] - lz.sum(), want, rtol=1e-9, atol=1e-10)
    assert np.all(e_np[cnt == 0] == 0.0)


def _reference_setup(rng):
    """The reference's fixture: Matern-1/2 (2, 2.25), two points, noise 1, z = x + 1e-10, sites seeded from one lr = 1 step of the
    sparse CVI model (here the oracle's NumPy SparseCVIGaussianProcess: ours needs the device; tests/test_gpu_spep.py seeds from ours)."""
    import torch
    import vidp_amd  # noqa: F401
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Gaussian, PEPScalarLikelihood
    from vidp_amd.sparse_pep import SparsePowerExpectationPropagation
    x = np.sort(rng.uniform(0.0, 3.0, 2))
    y = rng.normal(size=(2, 1))
    z = x + 1e-10
    sep = SparsePowerExpectationPropagation(K.Matern12(2.0, 2.25), torch.from_numpy(z), PEPScalarLikelihood(Gaussian(1.0)),
                                            learning_rate=0.1, alpha=1.0)
    scvi = np_conditionals.SparseCVIGaussianProcess(np_kernels.Matern12(2.0, 2.25), z, np_models.GaussianLik(1.0), learning_rate=1.0)
    scvi.update_sites(x, y)
    sep.nat1, sep.nat2 = _T(scvi.nat1), _T(scvi.nat2)
    llh = np_models.gpr_log_likelihood(x, y, np_kernels.Matern12(2.0, 2.25), 1.0)
    return sep, (_T(x), _T(y)), y, llh


def test_reference_optimal_sites(rng):
    sep, data, y, llh = _reference_setup(rng)
    sep.learning_rate = 1.0
    sep.update_sites(data)
    sd = 1
    np.testing.assert_array_almost_equal(sep.nat1.numpy()[:-1, sd:], y, decimal=3)
    np.testing.assert_array_almost_equal(sep.nat2.numpy()[:-1, sd:, sd:], -0.5 * np.ones((2, 1, 1)), decimal=3)
    np.testing.assert_array_almost_equal(sep.log_norm.numpy()[:-1], -0.5 * y ** 2 - 0.5 * np.log(2.0 * np.pi), decimal=4)
    np.testing.assert_array_almost_equal(float(sep.energy(data)), llh, decimal=4)


def test_reference_log_norm(rng):
    sep, data, y, _ = _reference_setup(rng)
    np.testing.assert_array_almost_equal(sep.compute_log_norm(data).numpy()[:-1, None], -0.5 * y ** 2 - 0.5 * np.log(2.0 * np.pi),
                                         decimal=4)


def test_reference_convergence(rng):
    sep, data, _, llh = _reference_setup(rng)
    for _ in range(20):
        sep.update_sites(data)
    old1, old2 = sep.nat1.numpy().copy(), sep.nat2.numpy().copy()
    sep.update_sites(data)
    np.testing.assert_array_almost_equal(sep.nat1.numpy(), old1)
    np.testing.assert_array_almost_equal(sep.nat2.numpy(), old2)
    # 4 decimals, the figure of test_reference_optimal_sites: the conditional statistics of points 1e-10 from their inducing point
    # invert matrices of size ~1e-10 and keep about 6 digits
    np.testing.assert_array_almost_equal(float(sep.energy(data)), llh, decimal=4)


def _improper_case(rng):
    n, M1 = 4, 5
    A = rng.normal(size=(M1, n, n))
    S = A @ A.transpose(0, 2, 1) + n * np.eye(n)
    mu = rng.normal(size=(M1, n))
    cnt = np.array([2, 0, 3, 1, 2])
    seg = np.concatenate([[0], np.cumsum(cnt)])
    N = cnt.sum()
    w, c, y = rng.normal(size=(N, n)), rng.uniform(0.01, 0.1, N), rng.normal(size=N)
    nat1 = rng.normal(size=(M1, n))
    nat2 = -0.2 * np.linalg.inv(S)                    # consistent: Lam + 2 beta nat2 = (1 - 0.4 beta) Lam stays positive definite
    alpha = 0.9
    # interval 2: -2 (alpha / n_m) nat2 larger than S^-1 along one direction
    v = rng.normal(size=n)
    nat2[2] = -(np.linalg.inv(S[2]) + 3.0 * np.outer(v, v)) / (2.0 * alpha / cnt[2]) * 1.5
    return seg, w, c, y, mu, S, nat1, nat2, rng.normal(size=M1), alpha


def test_improper_cavity_skips_the_interval(rng):
    """A pair marginal inconsistent with its site (Lam_c indefinite): the interval keeps site and log_norm bit for bit, is counted
    with its n_m points and gets e = NaN, its neighbours update; torch route and NumPy model alike."""
    import vidp_amd  # noqa: F401
    from vidp_amd.sparse_pep import interval_update
    seg, w, c, y, mu, S, nat1, nat2, ln, alpha = _improper_case(rng)
    o1, o2, o3, oe, osk = np_spep.interval_update("gaussian", seg, w, c, y, mu, S, nat1, nat2, ln, 0.6, alpha, 0.7)
    idx = np.repeat(np.arange(5), np.diff(seg))
    t1, t2, t3, te, tsk = interval_update(_lik("gaussian"), alpha, 0.7, _T(idx).long(), _T(w), _T(c), _T(y), _T(mu), _T(S), _T(nat1),
                                          _T(nat2), _T(ln))
    for g1, g2, g3, ge, sk in ((o1, o2, o3, oe, osk), (t1.numpy(), t2.numpy(), t3.numpy(), te.numpy(), int(tsk))):
        assert sk == 3
        np.testing.assert_array_equal(g1[2], nat1[2])
        np.testing.assert_array_equal(g2[2], nat2[2])
        assert g3[2] == ln[2] and np.isnan(ge[2]) and np.isfinite(np.delete(ge, 2)).all() and ge[1] == 0.0
        for m in (0, 1, 3, 4):
            assert not np.array_equal(g2[m], nat2[m])
    np.testing.assert_allclose(t2.numpy(), o2, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(np.delete(te.numpy(), 2), np.delete(oe, 2), rtol=1e-10)
    # an interval without data takes the formula with an empty sum
    np.testing.assert_allclose(o2[1], (1 - 0.7 * alpha) * nat2[1], rtol=1e-14)


def test_validation():
    import torch
    import vidp_amd  # noqa: F401
    from vidp_amd import kernels as K
    from vidp_amd.sparse_pep import SparsePowerExpectationPropagation
    z = torch.linspace(0.0, 1.0, 5, dtype=torch.float64)
    mk = lambda **kw: SparsePowerExpectationPropagation(K.Matern12(1.0, 1.0), kw.pop("z", z), _lik("gaussian"), **kw)
    m = mk(alpha=0.5)
    assert tuple(m.nat1.shape) == (6, 2) and tuple(m.log_norm.shape) == (6, 1)
    np.testing.assert_array_equal(m.nat2.numpy(), np.tile(-1e-10 * np.eye(2), (6, 1, 1)))
    for bad in (dict(alpha=0.0), dict(alpha=1.5), dict(learning_rate=-0.1), dict(learning_rate=1.1)):
        with pytest.raises(ValueError):
            mk(**bad)
    with pytest.raises(NotImplementedError):
        mk(z=z.repeat(2, 1))
