"""
GPU tests of Power Expectation Propagation (vidp_amd.pep.PowerExpectationPropagation; kernels mfgm_pep_sites / mfgm_pep_tilted,
csrc/mfgm_pep.h): the kernels against the NumPy restatement tests/np_pep.py, selection, null outputs, energy mode and skipped points,
the native route against the torch route, the model against the dense NumPy model, the reference's convergence test, the known answer
of a Gaussian likelihood, the walkthrough's setup and step_graph replay.  fp64.
"""
import numpy as np
import pytest

from oracle import np_kernels
from tests import np_pep

pytestmark = pytest.mark.gpu

KINDS = {"gaussian": (3, 0.6), "bernoulli": (1, 1e-3), "poisson": (2, 1.3)}


@pytest.fixture(scope="module")
def amd():
    import torch
    import vidp_amd
    assert torch.cuda.is_available()
    vidp_amd._lib.load()
    return vidp_amd


def dev(x, dtype=np.float64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def host(x):
    return x.detach().cpu().numpy()


def _draws(rng, kind, n, alpha):
    mu = rng.uniform(-4, 4, size=n)
    v = 10.0 ** rng.uniform(-3, 0.5, size=n)
    if kind == "bernoulli":
        y = rng.choice([0.0, 1.0], size=n)
    elif kind == "poisson":
        mu = rng.uniform(-2, 2, size=n)
        y = rng.poisson(2.0, size=n).astype(np.float64)
    else:
        y = rng.normal(size=n)
    nat1 = rng.normal(size=n)
    nat2 = 0.5 * rng.uniform(-0.9, 2.0, size=n) / (alpha * v)     # lc = (1 + u) / v > 0
    return mu, v, y, nat1, nat2, rng.normal(size=n)


def pep_sites(amd, kind, param, alpha, lr, mu, v, y, n1, n2, ln, idx=None, want_e=True, want_ln=True):
    """Direct call of mfgm_pep_sites on device copies; returns host (nat1, nat2, lnorm, e, skipped)."""
    import torch
    from vidp_amd.packed import _ptr, _stream
    n = len(mu)
    b = [dev(a) for a in (mu, v, y, n1, n2, ln)]
    e = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    sk = torch.zeros(1, dtype=torch.int32, device="cuda")
    ix = None if idx is None else dev(idx, np.int64)
    amd._lib.check(amd._lib.load().mfgm_pep_sites(kind, n, _ptr(b[0]), _ptr(b[1]), _ptr(b[2]), param, alpha, lr, _ptr(ix),
                                                  0 if idx is None else len(idx), _ptr(b[3]), _ptr(b[4]), _ptr(b[5]) if want_ln else None,
                                                  _ptr(e) if want_e else None, _ptr(sk), _stream()), "mfgm_pep_sites")
    torch.cuda.synchronize()
    return host(b[3]), host(b[4]), host(b[5]), host(e), int(sk.item())


def _scales(kind, mu, v, y, n1, n2, ln, param, alpha, lr):
    """Error scales of the updated sites and e: sums of absolute terms, with the conditioning of L2 = 1/2 / (vc + 1/d2) and of
    d1/d2 - mc carried through."""
    mc, vc, _ = np_pep.cavity_f(mu, v, n1, n2, alpha)
    lz, d1, d2, sc = np_pep.tilted(kind, mc, vc, y, param, alpha)
    L1, L2 = np_pep.gradient_correction([mc, vc], [d1, d2])
    k2 = (vc + 1.0 / np.abs(d2)) / np.abs(vc + 1.0 / d2) * (1.0 + sc["d2"] / np.abs(d2))
    r = d1 / d2
    k1 = (np.abs(r) * (1.0 + sc["d1"] / np.maximum(np.abs(d1), 1e-300) + sc["d2"] / np.abs(d2)) + np.abs(mc)) / np.abs(r - mc)
    sL1, sL2 = np.abs(L1) * (1.0 + k2 + k1), np.abs(L2) * (1.0 + k2)
    se = np.abs(lz) + 1.0 + 0.5 * (np.abs(np.log(vc)) + mc * mc / vc + np.abs(np.log(v)) + mu * mu / v)
    s1 = np.abs((1 - lr) * n1) + lr * (np.abs((1 - alpha) * n1) + sL1)
    s2 = np.abs((1 - lr) * n2) + lr * (np.abs((1 - alpha) * n2) + sL2)
    s3 = np.abs((1 - lr) * ln) + lr * (np.abs((1 - alpha) * ln) + se)
    return s1, s2, s3, se


@pytest.mark.parametrize("alpha", [0.5, 0.9, 1.0])
@pytest.mark.parametrize("kind", ["gaussian", "bernoulli", "poisson"])
def test_kernel_matches_numpy(amd, rng, kind, alpha):
    """mfgm_pep_sites over 1e5 + 3 random points (all selected, lr = 0.7) against np_pep.site_update, and mfgm_pep_tilted against
    np_pep.tilted: 1e-12 of the sum of absolute terms of each quantity."""
    import torch
    from vidp_amd.packed import _ptr, _stream
    k, param = KINDS[kind]
    n = 100003
    mu, v, y, n1, n2, ln = _draws(rng, kind, n, alpha)
    g1, g2, g3, ge, sk = pep_sites(amd, k, param, alpha, 0.7, mu, v, y, n1, n2, ln)
    w1, w2, w3, we, ok = np_pep.site_update(kind, mu, v, y, n1, n2, ln, param, alpha, 0.7)
    assert ok.all() and sk == 0
    s1, s2, s3, se = _scales(kind, mu, v, y, n1, n2, ln, param, alpha, 0.7)
    for got, want, s in ((g1, w1, s1), (g2, w2, s2), (g3, w3, s3), (ge, we, se)):
        assert np.all(np.abs(got - want) <= 1e-12 * s), np.max(np.abs(got - want) / s)
    mc, vc, _ = np_pep.cavity_f(mu, v, n1, n2, alpha)
    lz, d1, d2, sc = np_pep.tilted(kind, mc, vc, y, param, alpha)
    b = [dev(a) for a in (mc, vc, y)]
    out = [torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(3)]
    amd._lib.check(amd._lib.load().mfgm_pep_tilted(k, n, *[_ptr(t) for t in b], param, alpha, *[_ptr(t) for t in out], _stream()),
                   "mfgm_pep_tilted")
    glz, gd1, gd2 = (host(t) for t in out)
    assert np.all(np.abs(glz - lz) <= 1e-12 * (1.0 + np.abs(lz)))
    assert np.all(np.abs(gd1 - d1) <= 1e-12 * (sc["d1"] + 1e-300))
    assert np.all(np.abs(gd2 - d2) <= 1e-12 * sc["d2"])


def test_selection_null_outputs_and_energy_mode(amd, rng):
    """Only the selected sites move; unselected sites, a null lnorm and a null e_out are left bit for bit; lr = 0 writes e alone."""
    k, param = KINDS["bernoulli"]
    n, alpha = 5000, 0.9
    mu, v, y, n1, n2, ln = _draws(rng, "bernoulli", n, alpha)
    idx = rng.choice(n, size=700, replace=False)
    g1, g2, g3, ge, _ = pep_sites(amd, k, param, alpha, 0.5, mu, v, y, n1, n2, ln, idx=idx, want_e=False, want_ln=False)
    w1, w2, _, _, _ = np_pep.site_update("bernoulli", mu, v, y, n1, n2, ln, param, alpha, 0.5)
    sel = np.zeros(n, bool)
    sel[idx] = True
    np.testing.assert_array_equal(g1[~sel], n1[~sel])
    np.testing.assert_array_equal(g2[~sel], n2[~sel])
    np.testing.assert_array_equal(g3, ln)
    assert np.all(ge == 7.0)
    np.testing.assert_allclose(g1[sel], w1[sel], rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(g2[sel], w2[sel], rtol=1e-10, atol=1e-10)
    # energy mode
    g1, g2, g3, ge, _ = pep_sites(amd, k, param, alpha, 0.0, mu, v, y, n1, n2, ln)
    np.testing.assert_array_equal(g1, n1)
    np.testing.assert_array_equal(g2, n2)
    np.testing.assert_array_equal(g3, ln)
    we = np_pep.site_update("bernoulli", mu, v, y, n1, n2, ln, param, alpha, 0.0)[3]
    np.testing.assert_allclose(ge, we, rtol=1e-12, atol=1e-12)


def test_improper_cavities_are_counted_and_skipped(amd, rng):
    """Constructed points with v <= 0 or 1/v + 2 alpha eta2 <= 0 keep their sites, get e = NaN and are counted; the rest update."""
    k, param = KINDS["poisson"]
    n, alpha = 1000, 0.5
    mu, v, y, n1, n2, ln = _draws(rng, "poisson", n, alpha)
    bad = rng.choice(n, size=37, replace=False)
    v[bad[:10]] = -np.abs(v[bad[:10]])
    v[bad[10:12]] = 0.0
    n2[bad[12:]] = -(1.0 + rng.uniform(size=25)) / (2.0 * alpha * v[bad[12:]])
    g1, g2, g3, ge, sk = pep_sites(amd, k, param, alpha, 1.0, mu, v, y, n1, n2, ln)
    assert sk == 37
    np.testing.assert_array_equal(g1[bad], n1[bad])
    np.testing.assert_array_equal(g2[bad], n2[bad])
    np.testing.assert_array_equal(g3[bad], ln[bad])
    assert np.isnan(ge[bad]).all()
    good = np.setdiff1d(np.arange(n), bad)
    w1, w2, _, _, ok = np_pep.site_update("poisson", mu, v, y, n1, n2, ln, param, alpha, 1.0)
    assert not ok[bad].any() and ok[good].all()
    np.testing.assert_allclose(g1[good], w1[good], rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("kind", ["gaussian", "bernoulli", "poisson"])
@pytest.mark.parametrize("alpha", [0.5, 1.0])
def test_native_route_matches_torch_route(amd, rng, kind, alpha):
    """PEPScalarLikelihood / PEPGaussian on device tensors (one launch of mfgm_pep_tilted) against the same call on CPU tensors (torch
    route: the formula and autograd twice)."""
    import torch
    from vidp_amd.likelihoods import Bernoulli, Gaussian, PEPGaussian, PEPScalarLikelihood, Poisson
    lik = {"gaussian": lambda: PEPGaussian(Gaussian(0.6)), "bernoulli": lambda: PEPScalarLikelihood(Bernoulli()),
           "poisson": lambda: PEPScalarLikelihood(Poisson(1.3))}[kind]()
    mc, vc, y = rng.uniform(-2, 2, 3000), 10.0 ** rng.uniform(-2, 0, 3000), rng.choice([0.0, 1.0, 2.0], 3000)
    c = [torch.from_numpy(a[:, None].copy()) for a in (mc, vc, y)]
    g = [t.cuda() for t in c]
    assert lik._native(*g) and not lik._native(*c)
    lz_n, (d1_n, d2_n) = lik.grad_log_expected_density(*g, alpha=alpha)
    lz_t, (d1_t, d2_t) = lik.grad_log_expected_density(*c, alpha=alpha)
    sc = np_pep.tilted(kind, mc, vc, y, lik.param, alpha)[3]
    np.testing.assert_allclose(host(lz_n), lz_t.numpy(), rtol=1e-12, atol=1e-12)
    assert np.all(np.abs(host(d1_n)[:, 0] - d1_t.numpy()[:, 0]) <= 1e-12 * (sc["d1"] + 1e-300))
    assert np.all(np.abs(host(d2_n)[:, 0] - d2_t.numpy()[:, 0]) <= 1e-12 * sc["d2"])


def _kernel(mod, name, scale=1.0):
    return {"m12": lambda: mod.Matern12(0.7, 1.3 * scale), "m32": lambda: mod.Matern32(1.1, 1.2 * scale),
            "m52": lambda: mod.Matern52(1.0, 1.5 * scale)}[name]()


def _data(rng, kind, n, t=None):
    # spacing 0.25 lengthscales: the posterior precision stays well conditioned (~1e5), so two fp64 factorisations agree to ~1e-12
    t = np.linspace(0.0, 20.0, n) if t is None else t
    f = 1.5 * np.sin(0.6 * t)
    if kind == "gaussian":
        y = f + np.sqrt(KINDS["gaussian"][1]) * rng.normal(size=n)
    elif kind == "bernoulli":
        y = (f + 0.5 * rng.normal(size=n) > 0).astype(np.float64)
    else:
        y = rng.poisson(np.exp(f)).astype(np.float64)
    return t, y


def _liks(kind):
    from vidp_amd.likelihoods import Bernoulli, Gaussian, PEPGaussian, PEPScalarLikelihood, Poisson
    return {"gaussian": lambda: PEPGaussian(Gaussian(KINDS["gaussian"][1])), "bernoulli": lambda: PEPScalarLikelihood(Bernoulli(1e-3)),
            "poisson": lambda: PEPScalarLikelihood(Poisson(1.3))}[kind]()


def _gpu_model(t, y, kernel, lik, alpha, lr):
    from vidp_amd.pep import PowerExpectationPropagation
    return PowerExpectationPropagation((dev(t), dev(y[:, None])), kernel, lik, learning_rate=lr, alpha=alpha)


def _models(rng, kind, kname, n, alpha, lr, t=None, y=None, kernels=None):
    """The device model and the dense NumPy model on the same data (T small: the NumPy model inverts T d x T d matrices)."""
    from vidp_amd import kernels as K
    t, yy = _data(rng, kind, n, t)
    y = yy if y is None else y
    # Poisson: a quarter of the prior variance -- at cavity variances ~ 1 the 20-point rule misjudges the tilted variance of a zero
    # count enough to give the site a negative precision (the rule's limit, the reference's too)
    sc = 0.25 if kind == "poisson" else 1.0
    kg, ko = (_kernel(K, kname, sc), _kernel(np_kernels, kname, sc)) if kernels is None else kernels
    return (_gpu_model(t, y, kg, _liks(kind), alpha, lr),
            np_pep.PowerExpectationPropagation(t, y, ko, kind, KINDS[kind][1], learning_rate=lr, alpha=alpha))


def _assert_model_close(g, o, tol):
    for a, b in ((g.sites.nat1[:, 0], o.nat1), (g.sites.nat2[:, 0, 0], o.nat2), (g.sites.log_norm[:, 0], o.log_norm)):
        np.testing.assert_allclose(host(a), b, rtol=tol, atol=tol * np.abs(b).max())
    np.testing.assert_allclose(float(g.elbo()), o.elbo(), rtol=tol)
    np.testing.assert_allclose(float(g.energy()), o.energy(), rtol=tol)


@pytest.mark.parametrize("lr", [0.5, 1.0])
@pytest.mark.parametrize("alpha", [0.5, 1.0])
@pytest.mark.parametrize("kind", ["gaussian", "bernoulli", "poisson"])
@pytest.mark.parametrize("kname", ["m12", "m32", "m52"])
def test_model_against_numpy(amd, rng, kname, kind, alpha, lr):
    """PowerExpectationPropagation follows the dense np_pep model over 10 seeded mini-batch steps (T = 80, batches of 20): sites,
    elbo() and energy() within 1e-9 after every step; no point is skipped."""
    g, o = _models(rng, kind, kname, 80, alpha, lr)
    for _ in range(10):
        idx = rng.permutation(80)[:20].reshape(-1, 1)
        g.update_sites(idx)
        o.update_sites(idx)
        _assert_model_close(g, o, 1e-9)
    assert g.num_skipped == 0


def test_model_generic_route_normalizers_and_cavity(amd, rng):
    """A likelihood without a native kind (the Bernoulli log density as a generic ScalarQuadratureLikelihood: the same rule at
    alpha = 0.9) takes the model's torch route and follows the native route; energy() equals dist_q.normalizer() -
    dist_p.normalizer() + sum e / alpha, the normalizers equal the dense ones, compute_cavity (the reference's state-space form) equals
    the f-space cavity, and site_indices of shape [k, 1] with duplicates select the same sites as [k]."""
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Bernoulli, PEPScalarLikelihood, ScalarQuadratureLikelihood
    a, o = _models(rng, "bernoulli", "m32", 60, 0.9, 0.5)
    y = host(a.observations)[:, 0]
    b = _gpu_model(o.t, y, K.Matern32(1.1, 1.2), PEPScalarLikelihood(ScalarQuadratureLikelihood(Bernoulli(1e-3)._log_prob)), 0.9, 0.5)
    fmu, fvar = b.predict_f_at_data()
    assert not b._native(fmu, fvar) and a._native(fmu, fvar)
    for _ in range(6):
        idx = rng.permutation(60)[:15]
        a.update_sites(np.concatenate([idx, idx[:4]]).reshape(-1, 1))
        b.update_sites(idx)
        o.update_sites(idx)
        for s, t in ((a.sites.nat1, b.sites.nat1), (a.sites.nat2, b.sites.nat2), (a.sites.log_norm, b.sites.log_norm)):
            np.testing.assert_allclose(host(s), host(t), rtol=1e-11, atol=1e-11 * float(t.abs().max()))
    np.testing.assert_allclose(float(b.energy()), float(a.energy()), rtol=1e-11)
    _assert_model_close(a, o, 1e-9)
    Pq, mu, _ = o.posterior()
    np.testing.assert_allclose(float(a.dist_q.normalizer()), np_pep.normalizer(Pq, mu), rtol=1e-10)
    np.testing.assert_allclose(float(a.dist_p.normalizer()), np_pep.normalizer(o.Pp, np.zeros(len(mu))), rtol=1e-10)
    want = float(a.dist_q.normalizer() - a.dist_p.normalizer() + a.compute_log_norm().sum() / a.alpha)
    np.testing.assert_allclose(float(a.energy()), want, rtol=1e-10)
    fmu, fvar = a.predict_f_at_data()
    mc, vc, _ = a._cavity_f(fmu, fvar)
    cm, cv = a.compute_cavity()
    np.testing.assert_allclose(host(cm), host(mc), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(host(cv), host(vc), rtol=1e-9)
    with pytest.raises(ValueError):
        a.update_sites([0, 60])
    with pytest.raises(ValueError):
        a.update_sites([-1])


@pytest.mark.parametrize("alpha,which", [(1.0, "scalar"), (1.0, "gaussian"), (0.5, "scalar"), (0.5, "gaussian")])
def test_convergence_of_pep_to_optimal(amd, rng, alpha, which):
    """The reference's test_convergence_of_pep_to_optimal: Matern-1/2 (lengthscale 2, variance 2.25), two points, noise 1, single-index
    steps; the sites reach (y / s^2, -1/2 / s^2, -1/2 y^2 / s^2 - 1/2 log 2 pi s^2) to 3 decimals.  20 steps at alpha = 1, as the
    reference; each visit contracts the error by 1 - alpha, so 40 at alpha = 0.5."""
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Gaussian, PEPGaussian, PEPScalarLikelihood
    from vidp_amd.pep import PowerExpectationPropagation
    t = np.sort(rng.uniform(0.0, 3.0, 2))
    y = rng.normal(size=(2, 1))
    lik = PEPScalarLikelihood(Gaussian(1.0)) if which == "scalar" else PEPGaussian(Gaussian(1.0))
    pep = PowerExpectationPropagation((dev(t), dev(y)), K.Matern12(2.0, 2.25), lik, learning_rate=1.0, alpha=alpha)
    for _ in range(20 if alpha == 1.0 else 40):
        pep.update_sites(rng.permutation(2)[:1].reshape(-1, 1))
    s2 = 1.0
    np.testing.assert_array_almost_equal(host(pep.sites.log_norm), -0.5 * y ** 2 / s2 - 0.5 * np.log(2.0 * np.pi * s2), decimal=3)
    np.testing.assert_array_almost_equal(host(pep.sites.nat1), y / s2, decimal=3)
    np.testing.assert_array_almost_equal(host(pep.sites.nat2), -0.5 / s2 * np.ones((2, 1, 1)), decimal=3)


@pytest.mark.parametrize("alpha", [0.5, 1.0])
def test_known_answer_gaussian(amd, rng, alpha):
    """T = 10 000, Matern-5/2, Gaussian likelihood: once the sites have converged, energy() and elbo() equal
    GaussianProcessRegression.log_likelihood() to 1e-8."""
    import torch
    from vidp_amd import kernels as K
    from vidp_amd.variational_cvi import GaussianProcessRegression
    T = 10000
    t = np.linspace(0.0, 2000.0, T)        # 0.2 lengthscales apart: at 0.02 the precision's conditioning alone costs ~5e-8
    y = 1.5 * np.sin(0.03 * t) + np.sqrt(0.6) * rng.normal(size=T)
    g = _gpu_model(t, y, K.Matern52(1.0, 1.5), _liks("gaussian"), alpha, 1.0)
    for _ in range(4 if alpha == 1.0 else 70):
        g.update_sites()
    gpr = GaussianProcessRegression((dev(t), dev(y[:, None])), K.Matern52(1.0, 1.5),
                                    chol_obs_covariance=torch.full((1, 1), np.sqrt(0.6), dtype=torch.float64, device="cuda"))
    want = float(gpr.log_likelihood())
    np.testing.assert_allclose(float(g.elbo()), want, rtol=1e-8)
    np.testing.assert_allclose(float(g.energy()), want, rtol=1e-8)
    assert g.num_skipped == 0


def test_walkthrough_setup(amd, rng):
    """The reference walkthrough's model: 300 Bernoulli points on [0, 1], Matern-5/2 (lengthscale 0.2, variance 5), alpha = 0.9,
    lr = 0.5, batches of 60 sites; 30 seeded steps against np_pep.  The points are 1/60 of a lengthscale apart and the posterior
    precision's condition number is ~1e15: two fp64 NumPy routes (inverse, Cholesky solve) of this same model already differ by 1e-6
    in the sites after 30 steps, so the agreement is held to 1e-5 (sites) and 1e-6 (elbo, energy; the two NumPy routes differ by 2e-8), not to 1e-8."""
    from vidp_amd import kernels as K
    t = np.linspace(0.0, 1.0, 300)
    y = (np.cos(20.0 * t) + rng.normal(size=300) > 0).astype(np.float64)
    g, o = _models(rng, "bernoulli", "m52", 300, 0.9, 0.5, t=t, y=y, kernels=(K.Matern52(0.2, 5.0), np_kernels.Matern52(0.2, 5.0)))
    for _ in range(30):
        idx = rng.permutation(300)[:60].reshape(-1, 1)
        g.update_sites(idx)
        o.update_sites(idx)
    for a, b in ((g.sites.nat1[:, 0], o.nat1), (g.sites.nat2[:, 0, 0], o.nat2), (g.sites.log_norm[:, 0], o.log_norm)):
        np.testing.assert_allclose(host(a), b, rtol=1e-5, atol=1e-5 * np.abs(b).max())
    np.testing.assert_allclose(float(g.elbo()), o.elbo(), rtol=1e-6)
    np.testing.assert_allclose(float(g.energy()), o.energy(), rtol=1e-6)
    assert g.num_skipped == 0


def test_step_graph_replays_equal_eager_steps(amd, rng):
    """PowerExpectationPropagation(Bernoulli).step_graph() at T = 100 000: 5 replays give the ELBOs and sites of 5 eager
    `update_sites(); elbo()` to 1e-12."""
    from vidp_amd import kernels as K
    T = 100000
    t = np.linspace(0.0, 1000.0, T)
    y = _data(rng, "bernoulli", T, t)[1]
    mk = lambda: _gpu_model(t, y, K.Matern52(0.5, 1.0), _liks("bernoulli"), 0.9, 0.5)
    a, b = mk(), mk()
    step = b.step_graph()
    want, got = [], []
    for _ in range(5):
        a.update_sites()
        want.append(float(a.elbo()))
        got.append(float(step()))
    b.dist_p.plan.check_info()
    assert np.all(np.isfinite(want))
    np.testing.assert_allclose(got, want, rtol=1e-12)
    for s, w in ((b.sites.nat1, a.sites.nat1), (b.sites.nat2, a.sites.nat2), (b.sites.log_norm, a.sites.log_norm)):
        np.testing.assert_allclose(host(s), host(w), rtol=1e-12, atol=1e-12 * float(w.abs().max()))
    np.testing.assert_allclose(float(b.energy()), float(a.energy()), rtol=1e-12)
