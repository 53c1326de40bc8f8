"""
Host tests of the multi-latent sparse CVI model (vidp_amd.multi_latent_variational.MultiLatentSparseCVI) and its two likelihoods
(vidp_amd.likelihoods.MultiStageLikelihood, HeteroskedasticGaussian) on the torch route with CPU tensors: the explicit site gradients
against autograd of the variational expectations, the MultiStage case table, log_prob against its formula, the model against the dense
NumPy model of tests/np_ml.py, the decomposition of MultiStage into three scalar sparse CVI models (a known answer), constructor
refusals, and the argument checks of the three C entry points (which return before any launch).
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import np_kernels
from tests import np_ml


T = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))


def _liks(kind):
    from vidp_amd.likelihoods import HeteroskedasticGaussian, MultiStageLikelihood
    if kind == "multistage":
        return MultiStageLikelihood(jitter=1e-3, binsize=1.3), np_ml.MultiStage(1e-3, 1.3)
    return HeteroskedasticGaussian(), np_ml.HetGauss()


def _marginals(rng, L, n=200):
    return rng.normal(size=(n, L)) * 1.2, rng.uniform(0.05, 1.5, size=(n, L))


def _ys(rng, kind, n):
    if kind == "multistage":
        return rng.choice([0.0, 1.0, 2.0, 3.0, 7.0, 2.5], size=n)
    return rng.normal(size=n) * 1.5


@pytest.mark.parametrize("kind", ["multistage", "hetgauss"])
def test_gradients_against_autograd(kind):
    """ve_gradients_expectation (explicit formulas; for the Bernoulli terms the derivatives of the rule) against torch autograd of
    variational_expectations, and both against tests/np_ml.py: 1e-12 of the sum of absolute terms."""
    rng = np.random.default_rng(1)
    lik, olik = _liks(kind)
    mu, var = _marginals(rng, lik.latent_dim)
    y = _ys(rng, kind, len(mu))
    Fm, Fv, Y = T(mu).requires_grad_(True), T(var).requires_grad_(True), T(y[:, None])
    ve = lik.variational_expectations(Fm, Fv, Y)
    assert tuple(ve.shape) == (len(mu),)
    dm, dv = torch.autograd.grad(ve.sum(), [Fm, Fv])
    g1, g2 = lik.ve_gradients_expectation(Fm.detach(), Fv.detach(), Y)
    assert tuple(g1.shape) == tuple(g2.shape) == mu.shape
    ove, og1, og2, sc = np_ml.grads_expectation(olik, mu, var, y)
    a1 = (dm - 2.0 * dv * Fm.detach()).numpy()
    for name, got, want, scale in (("ve", ve.detach().numpy(), ove, sc["ve"]), ("g1 (autograd)", a1, og1, sc["g1"]),
                                   ("g2 (autograd)", dv.numpy(), og2, sc["g2"]), ("g1", g1.numpy(), og1, sc["g1"]),
                                   ("g2", g2.numpy(), og2, sc["g2"]), ("g1 vs autograd", g1.numpy(), a1, sc["g1"]),
                                   ("g2 vs autograd", g2.numpy(), dv.numpy(), sc["g2"])):
        err = np.max(np.abs(got - want) / (1e-12 * scale + 1e-300))
        print(f"{kind} {name}: |got - want| / (1e-12 sum|terms|) = {err:.3e}")
        assert err <= 1.0
    assert float(g2.max()) <= 0.0 or kind == "multistage"


def test_hetgauss_curvature_is_never_positive():
    """Both g2 of the heteroskedastic Gaussian are <= 0 at every input (extreme ones included)."""
    from vidp_amd.likelihoods import HeteroskedasticGaussian
    rng = np.random.default_rng(2)
    mu = rng.normal(size=(500, 2)) * 8.0
    var = np.exp(rng.normal(size=(500, 2)) * 3.0)
    y = rng.normal(size=(500, 1)) * 10.0
    _, g2 = HeteroskedasticGaussian().ve_gradients_expectation(T(mu), T(var), T(y))
    assert float(g2.max()) <= 0.0


def test_multistage_case_table():
    """y == 0 touches latent 0 only, y == 1 latents 0 and 1, y >= 2 all three; y in {-1, 0.5, 1.5, NaN} gives zeros everywhere; every
    entry equals the scalar Bernoulli / Poisson likelihood of the case."""
    from vidp_amd.likelihoods import Bernoulli, MultiStageLikelihood, Poisson
    rng = np.random.default_rng(3)
    lik, bern, pois = MultiStageLikelihood(2e-3, 0.7), Bernoulli(2e-3), Poisson(0.7)
    ys = np.array([0.0, 1.0, 2.0, 5.0, -1.0, 0.5, 1.5, np.nan])
    mu, var = _marginals(rng, 3, len(ys))
    Fm, Fv, Y = T(mu), T(var), T(ys[:, None])
    ve = lik.variational_expectations(Fm, Fv, Y).numpy()
    g1, g2 = (g.numpy() for g in lik.ve_gradients_expectation(Fm, Fv, Y))
    lp = lik.log_prob(Fm, Y).numpy()
    assert np.all(ve[4:] == 0.0) and np.all(g1[4:] == 0.0) and np.all(g2[4:] == 0.0) and np.all(lp[4:] == 0.0)
    assert np.all(g1[0, 1:] == 0.0) and np.all(g2[0, 1:] == 0.0) and g1[1, 2] == 0.0 and g2[1, 2] == 0.0
    assert np.all(g2[:4, 0] != 0.0) and np.all(g2[1:4, 1] != 0.0) and np.all(g2[2:4, 2] != 0.0)

    def scalar(b, l, label):
        col = lambda a: T(a[:, l:l + 1])
        lab = T(label[:, None])
        h1, h2 = b.ve_gradients_expectation(col(mu), col(var), lab)
        return b.variational_expectations(col(mu)[:, None], col(var)[:, None], lab[:, None])[:, 0].numpy(), h1[:, 0].numpy(), h2[:, 0].numpy()

    b0 = scalar(bern, 0, (ys == 0).astype(np.float64))
    b1 = scalar(bern, 1, (ys == 1).astype(np.float64))
    p2 = scalar(pois, 2, np.where(ys >= 2, ys - 2.0, 0.0))
    want = np.array([b0[0][0], b0[0][1] + b1[0][1], b0[0][2] + b1[0][2] + p2[0][2], b0[0][3] + b1[0][3] + p2[0][3]])
    np.testing.assert_allclose(ve[:4], want, rtol=1e-13)
    for k, g in ((1, g1), (2, g2)):
        np.testing.assert_allclose(g[:4, 0], b0[k][:4], rtol=1e-12)
        np.testing.assert_allclose(g[1:4, 1], b1[k][1:4], rtol=1e-12)
        np.testing.assert_allclose(g[2:4, 2], p2[k][2:4], rtol=1e-12)


@pytest.mark.parametrize("kind", ["multistage", "hetgauss"])
def test_log_prob_and_sampling(kind):
    rng = np.random.default_rng(4)
    lik, olik = _liks(kind)
    F = rng.normal(size=(300, lik.latent_dim))
    y = _ys(rng, kind, 300)
    np.testing.assert_allclose(lik.log_prob(T(F), T(y[:, None])).numpy(), olik.log_prob(F, y), rtol=1e-13, atol=1e-14)
    s1, s2, s3 = lik.sample_y(T(F), seed=5), lik.sample_y(T(F), seed=5), lik.sample_y(T(F), seed=6)
    assert tuple(s1.shape) == (300, 1) and torch.equal(s1, s2) and not torch.equal(s1, s3)
    if kind == "multistage":
        s = s1.numpy()
        assert np.all(s >= 0) and np.all(s == np.round(s)) and {0.0, 1.0} <= set(s[:, 0]) and s.max() >= 2
    with pytest.raises(NotImplementedError):
        lik.predict_log_density(T(F), T(F), T(y[:, None]))
    with pytest.raises(NotImplementedError):
        lik.predict_mean_and_var(T(F), T(F))


multistage_data, hetgauss_data = np_ml.multistage_data, np_ml.hetgauss_data


def multistage_kernels(K):
    return [K.Matern32(1.0, 1.0), K.Matern32(0.8, 0.8), K.Matern12(1.0, 0.25)]


def hetgauss_kernels(K):
    return [K.Matern52(1.0, 1.0), K.Matern32(0.8, 0.5)]


@pytest.mark.parametrize("kind", ["multistage", "hetgauss"])
def test_torch_route_against_dense_numpy(kind):
    """40 inducing points 0.25 lengthscales apart, 600 points, twenty damped steps (lr = 0.5): sites, ELBO, predict_f_at_data and
    predict_f at new times against tests/np_ml.py at the project's model-level 1e-8."""
    from vidp_amd import kernels as K
    from vidp_amd.multi_latent_variational import MultiLatentSparseCVI
    rng = np.random.default_rng(7)
    z = 0.25 * np.arange(40.0)
    lik, olik = _liks(kind)
    t, y = (multistage_data if kind == "multistage" else hetgauss_data)(rng, z, 600)
    kids, okids = (multistage_kernels if kind == "multistage" else hetgauss_kernels)(K), (multistage_kernels if kind == "multistage"
                                                                                         else hetgauss_kernels)(np_kernels)
    m = MultiLatentSparseCVI(K.IndependentMultiOutput(kids), T(z), lik, learning_rate=0.5)
    o = np_ml.MultiLatentSparseCVI(okids, z, olik, learning_rate=0.5)
    data = (T(t), T(y))
    tol = 1e-8
    for step in range(20):
        m.update_sites(data)
        o.update_sites(t, y)
        np.testing.assert_allclose(m.nat1.numpy(), o.nat1, rtol=tol, atol=tol * np.abs(o.nat1).max())
        np.testing.assert_allclose(m.nat2.numpy(), o.nat2, rtol=tol, atol=tol * np.abs(o.nat2).max())
        em, eo = float(m.elbo(data)), o.elbo(t, y)
        if step in (0, 19):
            print(f"ml host {kind} step {step}: elbo torch {em!r} numpy {eo!r}")
        np.testing.assert_allclose(em, eo, rtol=tol)
    assert float(m.loss(data)) == -float(m.classic_elbo(data))
    tn = rng.uniform(z[0] - 0.5, z[-1] + 0.5, size=150)          # unsorted new times
    for tt, (fm, fv) in ((t, m.predict_f_at_data(data)), (tn, m.predict_f(T(tn)))):
        om, ov = o.predict_f(tt)
        assert tuple(fm.shape) == (len(tt), lik.latent_dim)
        np.testing.assert_allclose(fm.numpy(), om, rtol=tol, atol=tol)
        np.testing.assert_allclose(fv.numpy(), ov, rtol=tol, atol=tol)
    with pytest.raises(NotImplementedError):
        m.predict_log_density(data)


def scalar_model(kernel, z, lik, lr):
    """The scalar sparse CVI model on the inducing grid z with CPU tensors: SparseCVIGaussianProcess itself has no CPU route, its
    spatio-temporal subclass has one, and with ONE spatial inducing point of unit variance at the location of every data point
    (a_i = 1, no spatial residual) it is the scalar model with `kernel` exactly."""
    from vidp_amd import space_kernels as SK
    from vidp_amd.spatio_temporal_variational import SpatioTemporalSparseCVI
    return SpatioTemporalSparseCVI(T(np.zeros((1, 1))), T(z), SK.Matern32(1.0, 1.0), kernel, lik, learning_rate=lr)


def test_multistage_decomposes_into_three_scalar_models():
    """MultiStage's expectation is additive over latents, so the model equals three scalar sparse CVI models on the same inducing
    grid -- Bernoulli on all points with labels 1[y = 0] (kernel 0), Bernoulli on the points with y >= 1 with labels 1[y = 1]
    (kernel 1), Poisson on the points with y >= 2 with counts y - 2 (kernel 2): the site blocks of latent l equal model l's sites, the
    cross-latent blocks are exactly 0, ELBO = sum of the three ELBOs, at 1e-8 over twenty damped steps."""
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Bernoulli, MultiStageLikelihood, Poisson
    from vidp_amd.multi_latent_variational import MultiLatentSparseCVI
    rng = np.random.default_rng(11)
    z = 0.25 * np.arange(40.0)
    t, y = multistage_data(rng, z, 600)
    kids = multistage_kernels(K)
    m = MultiLatentSparseCVI(K.IndependentMultiOutput(kids), T(z), MultiStageLikelihood(1e-3, 1.3), learning_rate=0.5)
    yy = y[:, 0]
    subsets = [(np.ones(len(t), bool), (yy == 0).astype(np.float64)), (yy >= 1, (yy == 1).astype(np.float64)), (yy >= 2, yy - 2.0)]
    liks = [Bernoulli(1e-3), Bernoulli(1e-3), Poisson(1.3)]
    parts, pdata = [], []
    for k, lik, (sel, lab) in zip(multistage_kernels(K), liks, subsets):
        parts.append(scalar_model(k, z, lik, 0.5))
        pdata.append((T(np.stack([np.zeros(sel.sum()), t[sel]], 1)), T(lab[sel][:, None])))
    data = (T(t), T(y))
    dl = [k.state_dim for k in kids]
    D, off = sum(dl), np.concatenate([[0], np.cumsum(dl)])
    mask = np_ml.slots(dl)
    cross = (mask.T @ mask) == 0
    tol = 1e-8
    for step in range(20):
        m.update_sites(data)
        total = 0.0
        n1, n2 = m.nat1.numpy(), m.nat2.numpy()
        for l, (p, pd) in enumerate(zip(parts, pdata)):
            p.update_sites(pd)
            total += float(p.elbo(pd))
            sl = np.r_[off[l]:off[l + 1], D + off[l]:D + off[l + 1]]
            w1, w2 = p.nat1.numpy(), p.nat2.numpy()
            np.testing.assert_allclose(n1[:, sl], w1, rtol=tol, atol=tol * np.abs(w1).max())
            np.testing.assert_allclose(n2[:, sl][:, :, sl], w2, rtol=tol, atol=tol * np.abs(w2).max())
        assert np.all(n2[:, cross] == 0.0)
        np.testing.assert_allclose(float(m.elbo(data)), total, rtol=tol)
    print(f"decomposition: elbo {float(m.elbo(data))!r} sum of the three scalar models {total!r}")


def test_constructor_refusals():
    import vidp_amd
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Gaussian, HeteroskedasticGaussian, MultiStageLikelihood
    cls = vidp_amd.MultiLatentSparseCVI
    z = T(np.arange(5.0))
    k3, k2 = K.IndependentMultiOutput(multistage_kernels(K)), K.IndependentMultiOutput(hetgauss_kernels(K))
    with pytest.raises(NotImplementedError, match="mean_function"):
        cls(k3, z, MultiStageLikelihood(), mean_function=lambda t: t)
    with pytest.raises(NotImplementedError, match="shard"):
        cls(k3, z, MultiStageLikelihood(), shard=(0, 2))
    with pytest.raises(ValueError, match="must agree"):
        cls(k2, z, MultiStageLikelihood())
    with pytest.raises(ValueError, match="must agree"):
        cls(k3, z, HeteroskedasticGaussian())
    with pytest.raises(ValueError, match="must agree"):
        cls(k2, z, Gaussian(1.0))
    with pytest.raises(TypeError, match="IndependentMultiOutput"):
        cls(K.Sum(hetgauss_kernels(K)), z, HeteroskedasticGaussian())
    with pytest.raises(NotImplementedError, match="batched"):
        cls(k2, z[None].repeat(2, 1), HeteroskedasticGaussian())
    wide = K.IndependentMultiOutput([K.Sum([K.Matern52(1.0, 1.0)] * 6), K.Sum([K.Matern52(1.0, 1.0)] * 5)])
    with pytest.raises(ValueError, match="state dimension 33"):
        cls(wide, z, HeteroskedasticGaussian())
    pw = K.PiecewiseKernel([K.Matern32(1.0, 1.0), K.Matern32(2.0, 1.0)], T(np.array([2.0])))
    with pytest.raises(NotImplementedError, match="PiecewiseKernel"):
        cls(K.IndependentMultiOutput([pw, K.Matern32(1.0, 1.0)]), z, HeteroskedasticGaussian())

    class Varying(K.IndependentMultiOutput):
        def generate_emission_model(self, time_points):
            em = super().generate_emission_model(time_points)
            em.constant_matrix = None
            return em

    with pytest.raises(NotImplementedError, match="time-invariant"):
        cls(Varying(hetgauss_kernels(K)), z, HeteroskedasticGaussian())
    with pytest.raises(ValueError):
        MultiStageLikelihood(jitter=0.5)
    with pytest.raises(ValueError):
        MultiStageLikelihood(binsize=0.0)
    m = cls(k2, z, HeteroskedasticGaussian())
    assert m.latent_dim == 2 and m.kernel is k2 and m.nat1.shape == (6, 10) and m.nat2.shape == (6, 10, 10)
    with pytest.raises(NotImplementedError, match="device"):
        m.dist_q


def test_entry_points_check_their_arguments_without_a_gpu():
    """mfgm_ml_predict_lik / mfgm_ml_site_update / mfgm_ml_site_update_q return 1 before any launch for L outside 1 .. 8, a dl < 1, D
    outside 2 .. 32, a kind whose L does not fit, a parameter out of range, lr outside [0, 1] and a missing pointer when N > 0."""
    import vidp_amd
    lib = vidp_amd._lib.load()
    one = ctypes.c_void_p(8)          # a non-null pointer that is never dereferenced: every call below fails its checks first

    def ml(dl, M=4, N=3, L=None, seg=one, h=one, c=one, pm=one, pc=one):
        s = vidp_amd._lib.MlData()
        s.M, s.L, s.N = M, len(dl) if L is None else L, N
        for k, n in enumerate(dl[:8]):
            s.dl[k] = n
        s.seg, s.h, s.c, s.prior_mean, s.prior_cov = seg, h, c, pm, pc
        return s

    def lk(kind, p0=1e-3, p1=1.0):
        q = vidp_amd._lib.MlLik()
        q.kind, q.param[0], q.param[1] = kind, p0, p1
        return q

    def predict(s, q=None, y=None, mu=one, ve=None, g1=None):
        q = lk(0) if q is None else q
        return lib.mfgm_ml_predict_lik(ctypes.byref(s), ctypes.byref(q), y, mu, one, one, one, one, ve, g1, None, None)

    def update(s, lr=0.5, g1=one, nat2=one, packed=False):
        fn = lib.mfgm_ml_site_update_q if packed else lib.mfgm_ml_site_update
        return fn(ctypes.byref(s), g1, one, lr, one, nat2, None)

    bad_shapes = [dict(dl=[1]), dict(dl=[16, 17]), dict(dl=[2, 0]), dict(dl=[2, -1, 4]), dict(dl=[4] * 8, L=9), dict(dl=[2, 2], L=0),
                  dict(dl=[2 ** 30, 2 ** 30, 2 ** 30, 2 ** 30]), dict(dl=[33]), dict(dl=[2, 2], M=0), dict(dl=[2, 2], N=-1),
                  dict(dl=[2, 2], seg=None), dict(dl=[2, 2], h=None), dict(dl=[2, 2], c=None)]
    for kw in bad_shapes:
        s = ml(**kw)
        assert predict(s) == 1 and update(s) == 1 and update(s, packed=True) == 1, kw
    ok3, ok2 = ml([2, 1, 3]), ml([3, 2])
    for q in (lk(1), lk(3), lk(-1)):                                   # MultiStage needs L == 3; unknown kinds
        assert predict(ok2, q, y=one, ve=one) == 1
    assert predict(ok3, lk(2), y=one, ve=one) == 1                      # HetGauss needs L == 2
    for p0, p1 in ((-1e-3, 1.0), (0.5, 1.0), (float("nan"), 1.0), (1e-3, 0.0), (1e-3, -1.0), (1e-3, float("nan")), (1e-3, float("inf"))):
        assert predict(ok3, lk(1, p0, p1), y=one, ve=one) == 1, (p0, p1)
    assert predict(ok3, lk(1), y=None, ve=one) == 1                     # a likelihood needs y
    assert predict(ok3, lk(0), y=one) == 1 and predict(ok3, lk(0), ve=one) == 1 and predict(ok3, lk(0), g1=one) == 1
    assert predict(ok3, mu=None) == 1 and predict(ml([2, 1, 3], pm=None)) == 1 and predict(ml([2, 1, 3], pc=None)) == 1
    for lr in (-0.1, 1.5, float("nan")):
        assert update(ok3, lr=lr) == 1 and update(ok3, lr=lr, packed=True) == 1
    for packed in (False, True):
        assert update(ok3, g1=None, packed=packed) == 1 and update(ok3, nat2=None, packed=packed) == 1
    q0 = lk(0)
    assert lib.mfgm_ml_predict_lik(None, ctypes.byref(q0), None, one, one, one, one, one, None, None, None, None) == 1
    assert lib.mfgm_ml_predict_lik(ctypes.byref(ok3), None, None, one, one, one, one, one, None, None, None, None) == 1
    assert lib.mfgm_ml_site_update(None, one, one, 0.5, one, one, None) == 1
    # no data and no likelihood: nothing to do
    assert predict(ml([2, 1, 3], N=0, h=None, c=None)) == 0
