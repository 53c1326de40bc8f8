"""
Host tests of the panel sparse CVI model (vidp_amd.panel_variational_cvi.PanelSparseCVI) on the torch route with CPU tensors: the
model against the dense NumPy model of tests/np_panel.py looped over the series, B = 1 against the single-series NumPy model, a series
without observations, constructor and data refusals, and the argument checks of the three C entry points (mfgm_panel_theta /
mfgm_panel_predict_lik / mfgm_panel_site_update), which return before any launch.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import np_kernels
from tests import np_panel

T = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
TOL = 1e-8          # the project's model-level tolerance on a grid 0.25 lengthscales apart (tests/test_gpu_ml.py, for the reasons given there)


def _setup(name):
    """(torch kernel, oracle kernel, torch likelihood, oracle likelihood, data kind); no lengthscale exceeds 1."""
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Bernoulli, Gaussian, Poisson
    if name == "matern32-gaussian":
        return K.Matern32(1.0, 1.0), np_kernels.Matern32(1.0, 1.0), Gaussian(0.09), np_panel.likelihood("gaussian", 0.09), "gaussian"
    if name == "matern52-poisson":
        return K.Matern52(1.0, 0.8), np_kernels.Matern52(1.0, 0.8), Poisson(1.3), np_panel.likelihood("poisson", 1.3), "poisson"
    kids = lambda m: m.Sum([m.Matern32(0.8, 0.6), m.Matern52(1.0, 0.4)])
    return kids(K), kids(np_kernels), Bernoulli(1e-3), np_panel.likelihood("bernoulli", 1e-3), "bernoulli"


def _follow(m, o, t, y, data, steps=20):
    for step in range(steps):
        m.update_sites(data)
        o.update_sites(t, y)
        w1, w2 = o.nat1, o.nat2
        np.testing.assert_allclose(m.nat1.numpy(), w1, rtol=TOL, atol=TOL * np.abs(w1).max())
        np.testing.assert_allclose(m.nat2.numpy(), w2, rtol=TOL, atol=TOL * np.abs(w2).max())
        eb, eo = m.elbo_per_series(data).numpy(), o.elbo_per_series(t, y)
        np.testing.assert_allclose(eb, eo, rtol=TOL, atol=TOL)
        np.testing.assert_allclose(float(m.classic_elbo(data)), eo.sum(), rtol=TOL)
    return eb, eo


@pytest.mark.parametrize("name", ["matern32-gaussian", "matern52-poisson", "sum5-bernoulli"])
def test_torch_route_against_dense_numpy(name):
    """Four series, 14 inducing points 0.25 lengthscales apart, 45 points each with about 15 % of them absent, twenty damped steps
    (lr = 0.5): sites, per-series ELBOs, their sum and predict_f at unsorted new times against tests/np_panel.py at 1e-8."""
    import vidp_amd
    rng = np.random.default_rng(3)
    k, ok, lik, olik, kind = _setup(name)
    B, z = 4, 0.25 * np.arange(14.0)
    t, y = np_panel.panel_data(rng, kind, z, B, 45)
    assert np.isnan(y).sum() > 5
    m = vidp_amd.PanelSparseCVI(k, T(z), lik, B, learning_rate=0.5)
    o = np_panel.Panel(ok, z, olik, B, learning_rate=0.5)
    data = (T(t), T(y))
    assert not m._native()
    eb, eo = _follow(m, o, t, y, data)
    print(f"panel host {name}: per-series elbo torch {eb!r} numpy {eo!r}")
    assert float(m.loss(data)) == -float(m.classic_elbo(data))
    tn = rng.uniform(z[0] - 0.5, z[-1] + 0.5, size=(B, 30))          # unsorted new times
    fm, fv = m.predict_f(T(tn))
    om, ov = o.predict_f(tn)
    assert tuple(fm.shape) == tuple(fv.shape) == (B, 30, 1)
    np.testing.assert_allclose(fm.numpy()[..., 0], om, rtol=TOL, atol=TOL)
    np.testing.assert_allclose(fv.numpy()[..., 0], ov, rtol=TOL, atol=TOL)
    if kind != "gaussian":
        lp = m.predict_log_density((T(tn), T(np.ones((B, 30, 1)))))
        assert tuple(lp.shape) == (B, 30) and bool(torch.isfinite(lp).all())


def test_one_series_is_the_single_series_model():
    """B = 1, no absent point: the panel model is the single-series NumPy model."""
    import vidp_amd
    rng = np.random.default_rng(5)
    k, ok, lik, olik, kind = _setup("matern52-poisson")
    z = 0.25 * np.arange(10.0)
    t, y = np_panel.panel_data(rng, kind, z, 1, 60, absent=0.0)
    m = vidp_amd.PanelSparseCVI(k, T(z), lik, 1, learning_rate=0.5)
    o = np_panel.SeriesSparseCVI(ok, z, olik, learning_rate=0.5)
    data = (T(t), T(y))
    for _ in range(20):
        m.update_sites(data)
        o.update_sites(t[0], y[0, :, 0])
        np.testing.assert_allclose(m.nat1.numpy()[0], o.nat1, rtol=TOL, atol=TOL * np.abs(o.nat1).max())
        np.testing.assert_allclose(m.nat2.numpy()[0], o.nat2, rtol=TOL, atol=TOL * np.abs(o.nat2).max())
        np.testing.assert_allclose(float(m.classic_elbo(data)), o.elbo(t[0], y[0, :, 0]), rtol=TOL)


def test_series_without_observations_keeps_zero_sites():
    """A row whose observations are all NaN: its sites stay exactly zero and its bound is 0 - KL(p || p) = 0 to rounding; the other
    rows are what they are without it."""
    import vidp_amd
    rng = np.random.default_rng(6)
    k, ok, lik, olik, kind = _setup("sum5-bernoulli")
    z = 0.25 * np.arange(9.0)
    t, y = np_panel.panel_data(rng, kind, z, 3, 30)
    y[1] = np.nan
    m = vidp_amd.PanelSparseCVI(k, T(z), lik, 3, learning_rate=0.5)
    o = np_panel.Panel(ok, z, olik, 3, learning_rate=0.5)
    data = (T(t), T(y))
    eb, _ = _follow(m, o, t, y, data, steps=5)
    assert float(m.nat1[1].abs().max()) == 0.0 and float(m.nat2[1].abs().max()) == 0.0
    assert float(m.nat2[0].abs().max()) > 0.0
    print(f"panel host: bound of the series without observations {eb[1]!r}")
    assert abs(eb[1]) <= 1e-10


def test_cache_follows_the_sites():
    """Editing nat1 in place, or assigning it, moves the ELBO: the cached marginals and predictions are dropped."""
    import vidp_amd
    rng = np.random.default_rng(7)
    k, _, lik, _, kind = _setup("matern32-gaussian")
    z = 0.25 * np.arange(8.0)
    t, y = np_panel.panel_data(rng, kind, z, 2, 20)
    m = vidp_amd.PanelSparseCVI(k, T(z), lik, 2, learning_rate=0.5)
    data = (T(t), T(y))
    m.update_sites(data)
    e0 = float(m.classic_elbo(data))
    assert float(m.classic_elbo(data)) == e0
    m.nat1[0, 3, 0] += 0.5
    e1 = float(m.classic_elbo(data))
    assert e1 != e0
    m.nat1 = m.nat1 * 0.5
    assert float(m.classic_elbo(data)) != e1


def test_refusals():
    import vidp_amd
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Gaussian
    cls = vidp_amd.PanelSparseCVI
    z, k, lik = T(0.25 * np.arange(6.0)), K.Matern32(1.0, 1.0), Gaussian(0.1)
    with pytest.raises(NotImplementedError, match="mean_function"):
        cls(k, z, lik, 3, mean_function=lambda t: t)
    with pytest.raises(NotImplementedError, match="shard"):
        cls(k, z, lik, 3, shard=(0, 2))
    with pytest.raises(NotImplementedError, match="per-series kernels"):
        cls([k, k, k], z, lik, 3)
    with pytest.raises(NotImplementedError, match="per-series inducing grids"):
        cls(k, z[None].repeat(3, 1), lik, 3)
    pw = K.PiecewiseKernel([K.Matern32(1.0, 1.0), K.Matern32(2.0, 1.0)], T(np.array([0.7])))
    with pytest.raises(NotImplementedError, match="PiecewiseKernel"):
        cls(pw, z, lik, 3)
    with pytest.raises(ValueError, match="two inducing points"):
        cls(k, z[:1], lik, 3)
    with pytest.raises(ValueError, match="num_series"):
        cls(k, z, lik, 0)
    m = cls(k, z, lik, 3)
    assert m.kernel is k and m.likelihood is lik and m.nat1.shape == (3, 7, 4) and m.nat2.shape == (3, 7, 4, 4)
    with pytest.raises(NotImplementedError, match="out of scope"):
        m.elbo_and_grad(None)
    with pytest.raises(NotImplementedError, match="device"):
        m.dist_q
    with pytest.raises(NotImplementedError, match="device"):
        m.dist_p
    rng = np.random.default_rng(8)
    t = np.sort(rng.uniform(0, 1.2, size=(3, 10)), axis=1)
    y = rng.normal(size=(3, 10, 1))
    for bad_t in (t[0], t[:2], t[None]):
        with pytest.raises(ValueError, match="num_series"):
            m.update_sites((T(bad_t), T(y)))
    with pytest.raises(ValueError, match="observations"):
        m.update_sites((T(t), T(y[..., 0])))
    with pytest.raises(ValueError, match="observations"):
        m.classic_elbo((T(t), T(y[:, :9])))
    shuffled = t[:, ::-1].copy()
    with pytest.raises(ValueError, match="sorted"):
        m.update_sites((T(shuffled), T(y)))
    with pytest.raises(ValueError, match="sorted"):
        m.classic_elbo((T(shuffled), T(y)))
    fm, _ = m.predict_f(T(shuffled))          # predict_f takes any order
    assert tuple(fm.shape) == (3, 10, 1)
    tn = t.copy()
    tn[1, 4] = np.nan
    for call in (lambda d: m.update_sites(d), lambda d: m.classic_elbo(d), lambda d: m.predict_f(d[0])):
        with pytest.raises(ValueError, match="NaN"):
            call((T(tn), T(y)))


def test_entry_points_check_their_arguments_without_a_gpu():
    """The three entry points return 1 before any launch for d outside 1 .. 8, a wide plan or a plan of another shape, an unknown kind
    or a parameter out of range, lr outside [0, 1] and a missing pointer when there is a point to cover."""
    import vidp_amd
    lib = vidp_amd._lib.load()
    one = ctypes.c_void_p(8)          # a non-null pointer that is never dereferenced: every call below fails its checks first

    def plan(B, Tn, d):
        h = ctypes.c_void_p()
        assert lib.mfgm_plan_create(B, Tn, d, 0, 0, ctypes.byref(h)) == 0
        return h

    def pd(B=3, M=5, d=2, N=4, idx=one, seg=one, w=one, c=one, pm=one, pc=one):
        s = vidp_amd._lib.PanelData()
        s.B, s.M, s.d, s.N = B, M, d, N
        s.idx, s.seg, s.w, s.c, s.prior_mean, s.prior_cov = idx, seg, w, c, pm, pc
        return s

    ok_plan, wide, others = plan(3, 5, 2), plan(3, 5, 9), [plan(2, 5, 2), plan(3, 6, 2), plan(3, 5, 3)]

    def theta(h, nat1=one, nat2=one, plin=one, pdiag=one, psub=one, lin=one, diag=one, sub=one):
        return lib.mfgm_panel_theta(h, nat1, nat2, plin, pdiag, psub, lin, diag, sub, None)

    def predict(h, s, kind=0, param=0.0, y=None, x=one, Sig=one, Sub=one, fmu=one, fvar=one, ve=None, g1=None, g2=None, vs=None):
        return lib.mfgm_panel_predict_lik(h, ctypes.byref(s), kind, param, y, x, Sig, Sub, fmu, fvar, ve, g1, g2, vs, None)

    def update(s, g1=one, g2=one, lr=0.5, nat1=one, nat2=one):
        return lib.mfgm_panel_site_update(ctypes.byref(s), g1, g2, lr, nat1, nat2, None)

    assert theta(None) == 1 and theta(wide) == 1
    for name in ("nat1", "nat2", "pdiag", "psub", "lin", "diag", "sub"):
        assert theta(ok_plan, **{name: None}) == 1, name
    ok = pd()
    for kw in (dict(d=0), dict(d=9), dict(d=-1), dict(B=0), dict(M=0), dict(N=-1)):
        assert predict(ok_plan, pd(**kw)) == 1 and update(pd(**kw)) == 1, kw
    assert predict(wide, pd(d=9)) == 1 and predict(wide, ok) == 1 and predict(None, ok) == 1
    for h in others:
        assert predict(h, ok) == 1
    assert lib.mfgm_panel_predict_lik(ok_plan, None, 0, 0.0, None, one, one, one, one, one, None, None, None, None, None) == 1
    for kind, param in ((4, 1.0), (-1, 1.0), (1, -1e-3), (1, 0.5), (1, float("nan")), (2, 0.0), (2, -1.0), (2, float("nan")),
                        (2, float("inf")), (3, 0.0), (3, -0.1), (3, float("nan")), (3, float("inf"))):
        assert predict(ok_plan, ok, kind, param, y=one, ve=one) == 1, (kind, param)
    for kind, param in ((1, 1e-3), (2, 1.3), (3, 0.1)):
        assert predict(ok_plan, ok, kind, param, y=None, ve=one) == 1          # a likelihood needs y
    for name in ("y", "ve", "g1", "g2", "vs"):                                   # kind 0 takes none of them
        assert predict(ok_plan, ok, **{name: one}) == 1, name
    for name in ("idx", "w", "c", "pm", "pc"):
        assert predict(ok_plan, pd(**{name: None})) == 1, name
    for name in ("x", "Sig", "Sub"):
        assert predict(ok_plan, ok, **{name: None}) == 1, name
    for lr in (-0.1, 1.5, float("nan")):
        assert update(ok, lr=lr) == 1
    for name in ("g1", "g2", "nat1", "nat2"):
        assert update(ok, **{name: None}) == 1, name
    assert update(pd(seg=None)) == 1 and update(pd(w=None)) == 1
    assert lib.mfgm_panel_site_update(None, one, one, 0.5, one, one, None) == 1
    # no point and nothing to write: nothing to do
    assert predict(ok_plan, pd(N=0, idx=None, w=None, c=None)) == 0
    for h in [ok_plan, wide] + others:
        lib.mfgm_plan_destroy(h)
