"""
GPU tests of the scalar non-Gaussian likelihoods (vidp_amd.likelihoods.Bernoulli / Poisson; kernel mfgm_scalar_lik, csrc/mfgm_lik.h):
the kernel against the NumPy restatement tests/np_lik.py, the HIP route against the torch route, CVIGaussianProcess and
SparseCVIGaussianProcess with these likelihoods against the oracle models, stationarity of the classic ELBO at the CVI fixed point,
step_graph replay and the predictions.  fp64.
"""
import numpy as np
import pytest

from oracle import np_models
from tests import np_lik

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
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def host(x):
    return x.detach().cpu().numpy()


def lik_draws(rng, n, kind):
    mu = rng.uniform(-8, 8, size=n)
    var = 10.0 ** rng.uniform(-6, 2, size=n)
    if kind == 1:
        y = rng.choice([0.0, 1.0, 1.0, 0.0, 2.0, -1.0], size=n)
    else:
        mu, var = rng.uniform(-4, 4, size=n), 10.0 ** rng.uniform(-6, 1, size=n)
        y = rng.poisson(3.0, size=n).astype(np.float64)
    return mu, var, y


def scalar_lik(amd, kind, mu, var, y, param, outs="vgh"):
    """Direct call of mfgm_scalar_lik; outputs not asked for are passed as null and must keep their sentinel."""
    import torch
    from vidp_amd.packed import _ptr, _stream
    n = mu.numel()
    bufs = [torch.full((n,), 7.0, dtype=torch.float64, device="cuda") for _ in range(3)]
    ptrs = [_ptr(b) if c in outs else _ptr(None) for b, c in zip(bufs, "vgh")]
    amd._lib.check(amd._lib.load().mfgm_scalar_lik(kind, n, _ptr(mu), _ptr(var), _ptr(y), param, *ptrs, _stream()), "mfgm_scalar_lik")
    torch.cuda.synchronize()
    return [host(b) for b in bufs]


@pytest.mark.parametrize("kind,param", [(1, 1e-3), (1, 0.0), (2, 1.0), (2, 0.25)])
def test_kernel_matches_numpy(amd, rng, kind, param):
    """VE, g1, g2 of the kernel against np_lik over 1e5 + 3 random (mu, v, y) (not a multiple of the block), |mu| <= 8, v in [1e-6, 1e2]:
    1e-12 of the sum of absolute terms of each quantity (g1 = dmu - 2 dv mu can cancel, so it is measured against |dmu| + 2 |dv mu|).
    With the jitter j = 1e-3 the probabilities stay >= j and erfc's far tail enters only through j + c Phi; with j = 0 it does not, and
    the comparison is kept to the 1e-12 bound on the points where Phi(s X) stays above 1e-300 for every node."""
    n = 100_003
    mu, var, y = lik_draws(rng, n, kind)
    ref = np_lik.Bernoulli(param) if kind == 1 else np_lik.Poisson(param)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ve, dmu, dv, sc = ref.ve_and_grads(mu, var, y)
    keep = np.ones(n, dtype=bool)
    if kind == 1 and param == 0.0:
        X = np_lik.nodes(mu, var)
        s = np.where(y == 1, 1.0, -1.0)[:, None]
        keep = (np_lik.phi_cdf(s * X) > 1e-300).all(-1)
        assert keep.mean() > 0.5
    v, g1, g2 = scalar_lik(amd, kind, dev(mu), dev(var), dev(y), param)
    with np.errstate(invalid="ignore"):          # the points left out at j = 0 are NaN on both sides
        g1_ref = dmu - 2 * dv * mu
        g1_sc = sc["dmu"] + 2 * np.abs(mu) * sc["dv"]
    for got, want, scale, name in ((v, ve, sc["ve"], "ve"), (g2, dv, sc["dv"], "g2"), (g1, g1_ref, g1_sc, "g1")):
        err = np.abs(got[keep] - want[keep]) / scale[keep]
        assert np.all(np.isfinite(got[keep])), name
        assert err.max() <= 1e-12, f"{name}: worst {err.max():.3g} of the scale"


def test_kernel_null_outputs_and_arguments(amd, rng):
    import torch
    n = 1000
    mu, var, y = lik_draws(rng, n, 1)
    full = scalar_lik(amd, 1, dev(mu), dev(var), dev(y), 1e-3)
    for outs in ("v", "g", "h", "gh", ""):
        part = scalar_lik(amd, 1, dev(mu), dev(var), dev(y), 1e-3, outs)
        for k, c in enumerate("vgh"):
            if c in outs:
                np.testing.assert_array_equal(part[k], full[k])
            else:
                assert np.all(part[k] == 7.0)
    from vidp_amd.packed import _ptr, _stream
    lib = amd._lib.load()
    a = dev(mu)
    o = torch.empty_like(a)
    for kind, param in ((0, 1e-3), (3, 1.0), (1, 0.5), (1, -1e-3), (2, 0.0), (2, -1.0)):
        assert lib.mfgm_scalar_lik(kind, n, _ptr(a), _ptr(a), _ptr(a), param, _ptr(o), None, None, _stream()) == 1
    assert lib.mfgm_scalar_lik(1, n, None, _ptr(a), _ptr(a), 1e-3, _ptr(o), None, None, _stream()) == 1
    assert lib.mfgm_scalar_lik(1, 0, None, None, None, 1e-3, None, None, None, _stream()) == 0


@pytest.mark.parametrize("which", ["bernoulli", "poisson"])
def test_hip_route_matches_torch_route(amd, rng, which):
    """The same tensors through the native route and the torch route (inputs that require grad take the torch route): 1e-12."""
    from vidp_amd.likelihoods import Bernoulli, Poisson
    n = 20_000
    kind = 1 if which == "bernoulli" else 2
    mu, var, y = lik_draws(rng, n, kind)
    lik = Bernoulli() if kind == 1 else Poisson(0.8)
    ref = np_lik.Bernoulli() if kind == 1 else np_lik.Poisson(0.8)
    sc = ref.ve_and_grads(mu, var, y)[3]
    m, v, yy = dev(mu[:, None]), dev(var[:, None]), dev(y[:, None])
    assert lik._native(m, v, yy)
    ve_h = host(lik.variational_expectations(m, v, yy))
    g1_h, g2_h = (host(x)[:, 0] for x in lik.ve_gradients_expectation(m, v, yy))
    mg, vg = m.clone().requires_grad_(True), v.clone().requires_grad_(True)
    assert not lik._native(mg, vg, yy)
    ve_t = host(lik.variational_expectations(mg, vg, yy))
    g1_t, g2_t = (host(x)[:, 0] for x in lik.ve_gradients_expectation(mg, vg, yy))
    assert ve_h.shape == ve_t.shape == (n,)
    assert np.all(np.abs(ve_h - ve_t) <= 1e-12 * sc["ve"])
    assert np.all(np.abs(g2_h - g2_t) <= 1e-12 * sc["dv"])
    assert np.all(np.abs(g1_h - g1_t) <= 1e-12 * (sc["dmu"] + 2 * np.abs(mu) * sc["dv"]))
    s = lik.variational_expectations_sum(m, v, yy)
    assert s.is_cuda and s.dim() == 0
    np.testing.assert_allclose(float(s), ve_h.sum(), rtol=1e-12)


def _kernel(mod, kname):
    return {"m12": lambda: mod.Matern12(0.7, 1.3), "sum": lambda: mod.Sum([mod.Matern32(1.1, 0.7), mod.Matern12(0.5, 1.2)])}[kname]()


def _cls_data(rng, n, which, t=None):
    t = np.linspace(0.0, 4.0, n) if t is None else t
    f = 1.5 * np.sin(3 * t)
    if which == "bernoulli":
        y = (f + 0.5 * rng.normal(size=n) > 0).astype(np.float64)
    else:
        y = rng.poisson(np.exp(f)).astype(np.float64)
    return t, y[:, None]


def _liks(which):
    from vidp_amd.likelihoods import Bernoulli, Poisson
    return (Bernoulli(), np_lik.Bernoulli()) if which == "bernoulli" else (Poisson(1.3), np_lik.Poisson(1.3))


@pytest.mark.parametrize("which", ["bernoulli", "poisson"])
@pytest.mark.parametrize("kname", ["m12", "sum"])
def test_cvi_gp_against_oracle(amd, rng, which, kname):
    """CVIGaussianProcess with a non-Gaussian likelihood follows oracle/np_models.CVIGaussianProcess with np_lik for 10 damped steps
    (lr = 0.5): sites, elbo() and classic_elbo() within 1e-9."""
    from oracle import np_kernels
    from vidp_amd import kernels as K
    from vidp_amd.variational_cvi import CVIGaussianProcess
    t, y = _cls_data(rng, 24, which)
    glik, olik = _liks(which)
    g = CVIGaussianProcess((dev(t), dev(y)), _kernel(K, kname), glik, learning_rate=0.5)
    o = np_models.CVIGaussianProcess(t, y, _kernel(np_kernels, kname), olik, learning_rate=0.5)
    for _ in range(10):
        g.update_sites()
        o.update_sites()
        np.testing.assert_allclose(host(g.sites.nat1), o.nat1, rtol=1e-9, atol=1e-9 * np.abs(o.nat1).max())
        np.testing.assert_allclose(host(g.sites.nat2), o.nat2, rtol=1e-9, atol=1e-9 * np.abs(o.nat2).max())
        np.testing.assert_allclose(float(g.elbo()), o.elbo(), rtol=1e-9)
        np.testing.assert_allclose(float(g.classic_elbo()), o.classic_elbo(), rtol=1e-9)


def test_cvi_gp_classic_elbo_stationary_at_fixed_point(amd, rng):
    """The non-conjugate form of KA7's third clause: at the fixed point of the Bernoulli CVI iteration (sites from the HIP route) the
    gradient of classic_elbo_tape() (torch route, autograd) with respect to the sites vanishes."""
    import torch
    from vidp_amd import kernels as K
    from vidp_amd.variational_cvi import CVIGaussianProcess
    t, y = _cls_data(rng, 50, "bernoulli", t=np.sort(rng.uniform(0, 5, size=50)))
    g = CVIGaussianProcess((dev(t), dev(y)), K.Matern12(0.8, 1.5), _liks("bernoulli")[0], learning_rate=0.5)
    it, change = 0, np.inf
    while change >= 1e-11:
        a1, a2 = g.sites.nat1.clone(), g.sites.nat2.clone()
        g.update_sites()
        change = max(float((g.sites.nat1 - a1).abs().max()), float((g.sites.nat2 - a2).abs().max()))
        it += 1
        assert it <= 400, f"no fixed point after 400 iterations (last change {change:.3g})"
    e, (n1, n2) = g.classic_elbo_tape()
    np.testing.assert_allclose(float(e.detach()), float(g.classic_elbo()), rtol=1e-9)
    g1, g2 = torch.autograd.grad(e, [n1, n2])
    np.testing.assert_allclose(host(g1), 0.0, atol=1e-7)
    np.testing.assert_allclose(host(g2), 0.0, atol=1e-7)
    # away from the fixed point the gradient is not small
    h = CVIGaussianProcess((dev(t), dev(y)), K.Matern12(0.8, 1.5), _liks("bernoulli")[0], learning_rate=0.5)
    h.update_sites()
    e, (n1, n2) = h.classic_elbo_tape()
    assert float(torch.autograd.grad(e, [n1])[0].abs().max()) > 1e-3


@pytest.mark.parametrize("route", ["fused", "generic"])
@pytest.mark.parametrize("which", ["bernoulli", "poisson"])
def test_sparse_cvi_against_oracle(amd, rng, monkeypatch, route, which):
    """SparseCVIGaussianProcess with a non-Gaussian likelihood follows oracle/np_conditionals.SparseCVIGaussianProcess for 5 steps, on the
    fused sorted-data route and on the generic route (VIDP_FUSED_SPARSE=0)."""
    from oracle import np_conditionals as npc, np_kernels
    from vidp_amd import kernels as K
    from vidp_amd.sparse_variational_cvi import SparseCVIGaussianProcess
    if route == "generic":
        monkeypatch.setenv("VIDP_FUSED_SPARSE", "0")
    t, y = _cls_data(rng, 40, which, t=np.linspace(0.0, 1.0, 40))
    z = np.linspace(-0.1, 1.1, 9)
    glik, olik = _liks(which)
    mk = lambda m: m.Matern12(0.3, 1.5)
    g = SparseCVIGaussianProcess(mk(K), dev(z), glik, learning_rate=0.6)
    o = npc.SparseCVIGaussianProcess(mk(np_kernels), z, olik, learning_rate=0.6)
    data = (dev(t), dev(y))
    assert (g._data(data) is None) == (route == "generic")
    for _ in range(5):
        g.update_sites(data)
        o.update_sites(t, y)
        np.testing.assert_allclose(host(g.nat1), o.nat1, rtol=1e-9, atol=1e-9 * np.abs(o.nat1).max())
        np.testing.assert_allclose(host(g.nat2), o.nat2, rtol=1e-9, atol=1e-9 * np.abs(o.nat2).max())
        np.testing.assert_allclose(float(g.classic_elbo(data)), o.classic_elbo(t, y), rtol=1e-9)
    # predictions at new points
    tn = np.sort(rng.uniform(-0.2, 1.2, size=11))
    tn_, yn = _cls_data(rng, 11, which, t=tn)
    omu, ovar = npc.predict_f(o.dist_q, mk(np_kernels), z, tn)
    np.testing.assert_allclose(host(g.predict_log_density((dev(tn), dev(yn)))), olik.predict_log_density(omu, ovar, yn), rtol=1e-8)


def test_cvi_step_graph_replays_equal_eager_steps(amd, rng):
    """CVIGaussianProcess(Bernoulli).step_graph(): k replays give the ELBOs and sites of k eager `update_sites(); elbo()` bit for bit.
    The captured step factorises the current sites inside update_sites (it does not reuse the factorisation elbo() left behind, see
    step_graph), so the bitwise reference is the eager step on that same order -- the plan's epoch advanced before each update_sites, as a
    replay does; the eager step with the shortcut is held to 1e-12."""
    from vidp_amd import kernels as K
    from vidp_amd.variational_cvi import CVIGaussianProcess
    t, y = _cls_data(rng, 3000, "bernoulli", t=np.linspace(0.0, 30.0, 3000))
    mk = lambda: CVIGaussianProcess((dev(t), dev(y)), K.Matern52(0.5, 1.0), _liks("bernoulli")[0], learning_rate=0.5)
    a, b, c = mk(), mk(), mk()
    step = b.step_graph()
    want, got, short = [], [], []
    for _ in range(6):
        a.dist_p.plan.epoch += 1
        a.update_sites()
        want.append(float(a.elbo()))
        c.update_sites()
        short.append(float(c.elbo()))
        got.append(float(step()))
    b.dist_p.plan.check_info()
    assert np.all(np.isfinite(want))
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(host(b.sites.nat1), host(a.sites.nat1))
    np.testing.assert_array_equal(host(b.sites.nat2), host(a.sites.nat2))
    np.testing.assert_allclose(short, want, rtol=1e-12)
    np.testing.assert_allclose(host(c.sites.nat1), host(a.sites.nat1), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("which", ["bernoulli", "poisson"])
def test_predictions(amd, rng, which):
    """CVIGaussianProcess.predict_log_density and AnalyticPosteriorProcess.predict_y with these likelihoods against np_lik on the oracle's
    predict_f."""
    from oracle import np_conditionals as npc, np_kernels
    from vidp_amd import kernels as K
    from vidp_amd.posterior import AnalyticPosteriorProcess
    from vidp_amd.variational_cvi import CVIGaussianProcess
    t, y = _cls_data(rng, 30, which)
    glik, olik = _liks(which)
    g = CVIGaussianProcess((dev(t), dev(y)), K.Matern12(0.7, 1.3), glik, learning_rate=0.5)
    o = np_models.CVIGaussianProcess(t, y, np_kernels.Matern12(0.7, 1.3), olik, learning_rate=0.5)
    for _ in range(4):
        g.update_sites()
        o.update_sites()
    tn = np.sort(rng.uniform(-0.5, 4.5, size=13))
    _, yn = _cls_data(rng, 13, which, t=tn)
    omu, ovar = npc.predict_f(o.dist_q, np_kernels.Matern12(0.7, 1.3), t, tn)
    lpd = host(g.predict_log_density((dev(tn), dev(yn))))
    assert lpd.shape == (13,)
    np.testing.assert_allclose(lpd, olik.predict_log_density(omu, ovar, yn), rtol=1e-8)
    post = AnalyticPosteriorProcess(g.dist_q, K.Matern12(0.7, 1.3), dev(t), glik)
    ym, yv = post.predict_y(dev(tn))
    om, ov = olik.predict_mean_and_var(omu, ovar)
    np.testing.assert_allclose(host(ym), om, rtol=1e-8)
    np.testing.assert_allclose(host(yv), ov, rtol=1e-8)
    assert type(g.posterior).__name__ == "ConditionalProcess"
