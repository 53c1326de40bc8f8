"""
GPU tests of the mean functions (vidp_amd.mean_function; kernels k_action_local / _ends / _apply / _mean, csrc/mfgm_mean.h; entry points
mfgm_action_coefficients / mfgm_action_mean) against the long-double restatement tests/np_mean.py, and of the models that take one:
GaussianProcessRegression, CVIGaussianProcess and SparseCVIGaussianProcess.  fp64.

Kernels: state dimensions 1 .. 8 through the trees of np_mean.tree, K in {1, 2, 5, 9, 70} actions, seg_len in {0, 1, 4, 64}, B in {1, 3}
with a grid per chain, gaps with exact ties and one gap of 50 lengthscales, unordered query points before the first action, on every
action time, one ulp above each, far beyond the last and random ones (130 of them; 2 K + 10 = 150 at K = 70, where the listed points
alone are 142).  Coefficients and means are held to 1e-12 of the absolute-value recurrence per entry.
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import np_kernels
from tests import np_kernels_ext as E
from tests import np_mean as NM

pytestmark = pytest.mark.gpu

BOUND = 1e-12
KS = (1, 2, 5, 9, 70)
SEGS = (0, 1, 4, 64)


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


def _grid(rng, Kn):
    """Action times of one chain: gaps in [0.05, 0.5], exact ties, one gap of 50 lengthscales (the longest is 1.3)."""
    gaps = rng.uniform(0.05, 0.5, size=Kn)
    if Kn >= 5:
        gaps[2] = 0.0
        gaps[3] = 65.0
    elif Kn == 2:
        gaps[1] = 65.0
    if Kn >= 9:
        gaps[6] = gaps[7] = 0.0              # three actions on one time
    return rng.uniform(0.0, 5.0) + np.cumsum(gaps)


def _queries(rng, t):
    Kn = t.size
    N = max(130, 2 * Kn + 10)
    fixed = np.concatenate([[t[0] - 1.0, np.nextafter(t[0], -np.inf)], t, np.nextafter(t, np.inf), [t[-1] + 40.0]])
    tq = np.concatenate([fixed, rng.uniform(t[0] - 0.5, t[-1] + 1.0, size=N - fixed.size)])
    return rng.permutation(tq)


@functools.lru_cache(maxsize=None)
def case(d, kind, Kn):
    """Inputs of three chains and their long-double reference, computed once per (d, kind, K): the device is handed the fp64 rhs and
    shift that the reference starts from."""
    rng = np.random.default_rng(1000 * d + 10 * Kn + (kind == "step"))
    ok = NM.tree(d, np_kernels, E)
    t = np.stack([_grid(rng, Kn) for _ in range(3)])
    u = rng.normal(size=(3, Kn, d))
    tq = np.stack([_queries(rng, t[b]) for b in range(3)])
    rhs, shift = u, None
    if kind == "step":
        parts = [NM.step_rhs(ok, u[b]) for b in range(3)]
        rhs = np.stack([p[0] for p in parts]).astype(np.float64)
        shift = np.stack([p[1] for p in parts]).astype(np.float64)
    h = NM.emission(ok)
    ref = []
    for b in range(3):
        c, s = NM.coefficients(ok, t[b], rhs[b])
        mu, ms = NM.evaluate(ok, t[b], c, s, None if shift is None else shift[b], tq[b])
        ref.append(dict(coef=c, scale=s, mu=mu, mu_scale=ms, f=mu @ h, f_scale=ms @ np.abs(h)))
    return dict(t=t, u=u, tq=tq, rhs=rhs, shift=shift, ref=ref, h=h.astype(np.float64))


def _err(got, ref, scale):
    """max |got - ref| / scale; where the scale is zero the entry must be exactly zero."""
    got = np.asarray(got, dtype=NM.LD)
    assert np.all(got[scale == 0] == 0)
    pos = scale > 0
    return float(np.max(np.abs(got - ref)[pos] / scale[pos])) if pos.any() else 0.0


def native_coefficients(amd, kt, t, rhs, seg_len, alias=False):
    import torch
    from vidp_amd.packed import _ptr, _stream
    lib = amd._lib.load()
    B, Kn, d = rhs.shape
    n = lib.mfgm_action_workspace_doubles(B, Kn, d, seg_len)
    seg = seg_len if seg_len > 0 else next(s for s in range(1, Kn + 1) if s * s >= Kn)
    assert n == B * -(-Kn // seg) * d
    ws = torch.full((n + 4,), 7.0, dtype=torch.float64, device="cuda")
    src = rhs.clone()
    coef = src if alias else torch.full_like(rhs, 7.0)
    amd._lib.check(lib.mfgm_action_coefficients(ctypes.byref(kt), B, Kn, seg_len, _ptr(t), _ptr(src), _ptr(coef), _ptr(ws), _stream()),
                   "mfgm_action_coefficients")
    torch.cuda.synchronize()
    assert bool((ws[n:] == 7.0).all())                   # nothing past the workspace the size function asked for
    if not alias:
        assert torch.equal(src, rhs)
    return coef


def native_mean(amd, kt, t, coef, shift, tq, h, outs="sf"):
    import torch
    from vidp_amd.packed import _ptr, _stream
    lib = amd._lib.load()
    B, Kn, d = coef.shape
    N = tq.shape[1]
    state = torch.full((B, N, d), 7.0, dtype=torch.float64, device="cuda")
    f = torch.full((B, N), 7.0, dtype=torch.float64, device="cuda")
    hrow = (ctypes.c_double * d)(*h.tolist())
    amd._lib.check(lib.mfgm_action_mean(ctypes.byref(kt), B, Kn, N, _ptr(t), _ptr(coef), _ptr(shift), _ptr(tq),
                                        ctypes.cast(hrow, ctypes.c_void_p), _ptr(state) if "s" in outs else None,
                                        _ptr(f) if "f" in outs else None, _stream()), "mfgm_action_mean")
    torch.cuda.synchronize()
    return state, f


@pytest.mark.parametrize("kind", ["impulse", "step"])
@pytest.mark.parametrize("d", range(1, 9))
def test_kernels_against_the_restatement(amd, d, kind):
    """Coefficients and means of the native entry points within 1e-12 of the absolute-value recurrence, for every K, seg_len and B;
    two calls and the aliased call give identical bits; each optional output alone equals the pair."""
    import torch
    from vidp_amd import kernels as K
    gk = NM.tree(d, K, K)
    kt = gk._terms_struct()
    worst_c = worst_m = 0.0
    for Kn in KS:
        cs = case(d, kind, Kn)
        for B in (1, 3):
            t, rhs, tq = dev(cs["t"][:B]), dev(cs["rhs"][:B]), dev(cs["tq"][:B])
            shift = None if cs["shift"] is None else dev(cs["shift"][:B])
            for seg in SEGS:
                coef = native_coefficients(amd, kt, t, rhs, seg)
                assert torch.equal(coef, native_coefficients(amd, kt, t, rhs, seg))
                assert torch.equal(coef, native_coefficients(amd, kt, t, rhs, seg, alias=True))
                state, f = native_mean(amd, kt, t, coef, shift, tq, cs["h"])
                for b in range(B):
                    r = cs["ref"][b]
                    worst_c = max(worst_c, _err(host(coef[b]), r["coef"], r["scale"]))
                    worst_m = max(worst_m, _err(host(state[b]), r["mu"], r["mu_scale"]), _err(host(f[b]), r["f"], r["f_scale"]))
                if seg == 0:
                    s2, f2 = native_mean(amd, kt, t, coef, shift, tq, cs["h"])
                    assert torch.equal(s2, state) and torch.equal(f2, f)
                    s1, f1 = native_mean(amd, kt, t, coef, shift, tq, cs["h"], outs="s")
                    assert torch.equal(s1, state) and bool((f1 == 7.0).all())
                    s1, f1 = native_mean(amd, kt, t, coef, shift, tq, cs["h"], outs="f")
                    assert torch.equal(f1, f) and bool((s1 == 7.0).all())
                    s1, f1 = native_mean(amd, kt, t, coef, shift, tq, cs["h"], outs="")
                    assert bool((s1 == 7.0).all()) and bool((f1 == 7.0).all())
    print(f"d={d} {kind}: worst coefficient error {worst_c:.3g}, worst mean error {worst_m:.3g} of the absolute-value scale")
    assert worst_c <= BOUND and worst_m <= BOUND


@pytest.mark.parametrize("kind", ["impulse", "step"])
@pytest.mark.parametrize("d", [3, 5, 8])
def test_an_action_is_not_seen_at_its_own_time(amd, d, kind):
    """The mean on an action time t_k is, bit for bit, the mean of the actions strictly before t_k alone (ties included): zero when
    there is none, otherwise what the entry points give for the truncated action list (the same seg_len, so the same grouping)."""
    import torch
    from vidp_amd import kernels as K
    kt = NM.tree(d, K, K)._terms_struct()
    cs = case(d, kind, 9)
    t, rhs = cs["t"][:1], cs["rhs"][:1]
    shift = None if cs["shift"] is None else cs["shift"][:1]
    coef = native_coefficients(amd, kt, dev(t), dev(rhs), 4)
    on = native_mean(amd, kt, dev(t), coef, None if shift is None else dev(shift), dev(t), cs["h"])
    seen = 0
    for k in range(9):
        j = int(np.searchsorted(t[0], t[0, k], side="left"))
        if j == 0:
            assert bool((on[0][0, k] == 0).all()) and float(on[1][0, k]) == 0.0
            continue
        cj = native_coefficients(amd, kt, dev(t[:, :j]), dev(rhs[:, :j]), 4)
        assert torch.equal(cj, coef[:, :j])
        tr = native_mean(amd, kt, dev(t[:, :j]), cj, None if shift is None else dev(shift[:, :j]), dev(t[:, k:k + 1]), cs["h"])
        assert torch.equal(tr[0][0, 0], on[0][0, k]) and torch.equal(tr[1][0, 0], on[1][0, k])
        seen += 1
    assert seen >= 7


@pytest.mark.parametrize("kind", ["impulse", "step"])
@pytest.mark.parametrize("d", range(1, 9))
def test_classes_on_the_device(amd, d, kind, monkeypatch):
    """ImpulseMeanFunction / StepMeanFunction on CUDA tensors (the native route, the fp64 solve against the generator included) against
    the restatement from the perturbations, batched and one chain; the torch route on the device (VIDP_NATIVE_MEAN=0) agrees."""
    from vidp_amd import kernels as K
    from vidp_amd import mean_function as MF
    cls = MF.ImpulseMeanFunction if kind == "impulse" else MF.StepMeanFunction
    gk, ok = NM.tree(d, K, K), NM.tree(d, np_kernels, E)
    cs = case(d, kind, 70)
    refs = [NM.mean(ok, kind, cs["t"][b], cs["u"][b], cs["tq"][b]) for b in range(3)]
    m = cls(dev(cs["t"]), dev(cs["u"]), gk)
    assert m._native(dev(cs["tq"]).device) is not None
    state, f = host(m.state_mean(dev(cs["tq"]))), host(m(dev(cs["tq"])))
    assert state.shape == (3, 150, d) and f.shape == (3, 150, 1)
    worst = max(max(_err(state[b], refs[b]["mu"], refs[b]["mu_scale"]), _err(f[b, :, 0], refs[b]["f"], refs[b]["f_scale"]))
                for b in range(3))
    one = cls(dev(cs["t"][1]), dev(cs["u"][1]), gk)
    np.testing.assert_array_equal(host(one(dev(cs["tq"][1]))), f[1])
    monkeypatch.setenv("VIDP_NATIVE_MEAN", "0")
    slow = cls(dev(cs["t"]), dev(cs["u"]), gk)
    assert slow._native(dev(cs["tq"]).device) is None
    ft = host(slow(dev(cs["tq"])))
    worst_t = max(_err(ft[b, :, 0], refs[b]["f"], refs[b]["f_scale"]) for b in range(3))
    print(f"d={d} {kind}: classes worst {worst:.3g} (native), {worst_t:.3g} (torch route) of the absolute-value scale")
    assert worst <= BOUND and worst_t <= BOUND


# ---- models ------------------------------------------------------------------------------------------------------------------------------
NOISE = 0.3
TA = np.array([0.7, 2.0, 3.1, 3.1, 6.2])          # K = 5 step actions (one tie)


def _grid40(rng):
    """T = 40 time points of the dense models: a jittered grid whose gaps stay above 0.16 (on gaps far below the lengthscales
    Q = Pinf - A Pinf A^T cancels and the prior is not positive definite in fp64)."""
    return np.linspace(0.0, 8.0, 40) + rng.uniform(-0.02, 0.02, size=40)


def _step_setup(rng, d):
    from vidp_amd import kernels as K
    mk = lambda: NM.tree(d, K, K)
    ok = NM.tree(d, np_kernels, E)
    u = 2.0 * rng.normal(size=(5, d))
    m_np = lambda t: NM.mean(ok, "step", TA, u, t)["f"].astype(np.float64)
    return mk, ok, u, m_np


def _step_mean(kernel, u):
    from vidp_amd.mean_function import StepMeanFunction
    return StepMeanFunction(dev(TA), dev(u), kernel)


def _dense_gp(ok, t, r, tn):
    """(log N(r | 0, K + s2 I), predictive mean and variance of the zero-mean GP at tn)."""
    Kd = E.dense_k(ok, t[:, None] - t[None, :]) + NOISE * np.eye(t.size)
    L = np.linalg.cholesky(Kd)
    a = np.linalg.solve(Kd, r)
    ll = -0.5 * r @ a - np.log(np.diag(L)).sum() - 0.5 * t.size * np.log(2.0 * np.pi)
    Ks = E.dense_k(ok, tn[:, None] - t[None, :])
    var = E.dense_k(ok, np.zeros(tn.size)) - np.einsum("ij,ji->i", Ks, np.linalg.solve(Kd, Ks.T))
    return ll, Ks @ a, var


@pytest.mark.parametrize("d", [3, 5])
def test_gpr_filters_the_residuals(amd, rng, d):
    """log_likelihood() and posterior.predict_f at 15 new points against the dense restatement -- y - m under N(0, K + s2 I), the
    predictive mean plus m at the new points -- at 1e-8.  (Before the mean functions the filter ran on the raw observations.)"""
    from vidp_amd.variational_cvi import GaussianProcessRegression
    mk, ok, u, m_np = _step_setup(rng, d)
    t = _grid40(rng)
    y = (m_np(t) + np.sin(2.0 * t) + 0.3 * rng.normal(size=40))[:, None]
    tn = rng.uniform(-0.5, 9.0, size=15)
    gk = mk()
    g = GaussianProcessRegression((dev(t), dev(y)), gk, chol_obs_covariance=dev(np.array([[np.sqrt(NOISE)]])),
                                  mean_function=_step_mean(gk, u))
    ll, pm, pv = _dense_gp(ok, t, y[:, 0] - m_np(t), tn)
    assert abs(_dense_gp(ok, t, y[:, 0], tn)[0] - ll) > 1e-3 * abs(ll)          # the mean matters on this data
    np.testing.assert_allclose(float(g.log_likelihood()), ll, rtol=1e-8)
    mu, var = g.posterior.predict_f(dev(tn))
    np.testing.assert_allclose(host(mu).reshape(-1), pm + m_np(tn), rtol=1e-8, atol=1e-8)
    np.testing.assert_allclose(host(var).reshape(-1), pv, rtol=1e-8, atol=1e-8)
    with pytest.raises(NotImplementedError, match="depends on the kernel"):
        g.log_likelihood_and_grad()


@pytest.mark.parametrize("d", [3, 5])
def test_cvi_with_a_gaussian_likelihood_is_gpr(amd, rng, d):
    """One update_sites() at learning_rate 1 with a Gaussian likelihood lands on the exact posterior: classic_elbo() and elbo() equal
    GaussianProcessRegression(mean_function=...).log_likelihood() at 1e-8.  (Before, the mean function was dropped.)"""
    from vidp_amd.likelihoods import Gaussian
    from vidp_amd.variational_cvi import CVIGaussianProcess, GaussianProcessRegression
    mk, ok, u, m_np = _step_setup(rng, d)
    t = _grid40(rng)
    y = (m_np(t) + np.sin(2.0 * t) + 0.3 * rng.normal(size=40))[:, None]
    gk = mk()
    gpr = GaussianProcessRegression((dev(t), dev(y)), gk, chol_obs_covariance=dev(np.array([[np.sqrt(NOISE)]])),
                                    mean_function=_step_mean(gk, u))
    ll = float(gpr.log_likelihood())
    np.testing.assert_allclose(ll, _dense_gp(ok, t, y[:, 0] - m_np(t), t[:1])[0], rtol=1e-8)
    for fused in ("1", "0"):
        ck = mk()
        c = CVIGaussianProcess((dev(t), dev(y)), ck, Gaussian(NOISE), mean_function=_step_mean(ck, u), learning_rate=1.0)
        if fused == "0":
            c._predict_f_fused = lambda: None                    # the unfused route of predict_f_at_data
        c.update_sites()
        np.testing.assert_allclose(float(c.classic_elbo()), ll, rtol=1e-8)
        np.testing.assert_allclose(float(c.elbo()), ll, rtol=1e-8)
    with pytest.raises(NotImplementedError, match="depends on the kernel"):
        c.classic_elbo_tape_hyper()


class LinearPlusStep:
    """m(t) = a t + the step response: a mean function put together in the test."""
    depends_on_kernel = True

    def __init__(self, a, step):
        self.a, self.step = a, step

    def __call__(self, t):
        return self.a * t[..., None] + self.step(t)

    def kernel_changed(self):
        self.step.kernel_changed()


def _site_targets(lik, fmu0, fvar0, m, y):
    """The gradients the sites move towards: those of the likelihood at (fmu0 + m, fvar0) with respect to [mu_f, var + mu_f^2], carried
    to the expectation parameters [mu_g, var + mu_g^2] of g = f - m, which the sites are on:  g1 = G1 + 2 G2 m,  g2 = G2  (at a
    Gaussian likelihood g1 = (y - m) / s2: the site of the residual, what makes elbo() the GPR likelihood above)."""
    G1, G2 = lik.ve_gradients_expectation(fmu0 + m, fvar0, y)
    return G1 + 2.0 * G2.reshape(G1.shape) * m, G2


@pytest.mark.parametrize("d", [3, 5])
def test_cvi_bernoulli_site_update(amd, rng, d):
    """One update_sites of CVIGaussianProcess(Bernoulli, linear-plus-step mean) equals (1 - rho) sites + rho targets, the targets
    from a mean-free twin model at the same sites: 1e-10."""
    from vidp_amd.likelihoods import Bernoulli
    from vidp_amd.stamps import wrote
    from vidp_amd.variational_cvi import CVIGaussianProcess
    mk, ok, u, m_np = _step_setup(rng, d)
    t = _grid40(rng)
    m = 0.2 * t + m_np(t)
    y = ((m + 1.5 * np.sin(3.0 * t) + 0.5 * rng.normal(size=40)) > 0).astype(np.float64)[:, None]
    rho = 0.4
    twin = CVIGaussianProcess((dev(t), dev(y)), mk(), Bernoulli(), learning_rate=rho)
    twin.update_sites()
    gk = mk()
    g = CVIGaussianProcess((dev(t), dev(y)), gk, Bernoulli(), mean_function=LinearPlusStep(0.2, _step_mean(gk, u)), learning_rate=rho)
    g.sites.nat1.copy_(twin.sites.nat1)
    g.sites.nat2.copy_(twin.sites.nat2)
    wrote(g.sites.nat1, g.sites.nat2)
    fmu0, fvar0 = twin.predict_f_at_data()
    g1, g2 = _site_targets(Bernoulli(), fmu0, fvar0, dev(m[:, None]), dev(y))
    want1 = (1 - rho) * twin.sites.nat1 + rho * g1
    want2 = (1 - rho) * twin.sites.nat2 + rho * g2.reshape(twin.sites.nat2.shape)
    np.testing.assert_allclose(host(g.predict_f_at_data()[0]), host(fmu0) + m[:, None], rtol=1e-12, atol=1e-12)
    # predict_log_density sees the shifted mean too
    tn = np.sort(rng.uniform(0.0, 8.0, size=7))
    yn = dev((rng.uniform(size=(7, 1)) > 0.5).astype(np.float64))
    fm, fv = twin.posterior.predict_f(dev(tn))
    np.testing.assert_allclose(host(g.predict_log_density((dev(tn), yn))),
                               host(Bernoulli().predict_log_density(fm + dev((0.2 * tn + m_np(tn))[:, None]), fv, yn)), rtol=1e-10)
    g.update_sites()
    np.testing.assert_allclose(host(g.sites.nat1), host(want1), rtol=0, atol=1e-10 * float(want1.abs().max()))
    np.testing.assert_allclose(host(g.sites.nat2), host(want2), rtol=0, atol=1e-10 * float(want2.abs().max()))
    assert float((g.sites.nat1 - ((1 - rho) * twin.sites.nat1 + rho * Bernoulli().ve_gradients_expectation(fmu0, fvar0, dev(y))[0]))
                 .abs().max()) > 1e-3            # the mean moves the update


def _sparse_data(rng, m_of_t):
    z = np.linspace(0.3, 7.7, 12)
    t = np.sort(rng.uniform(0.0, 8.0, size=60))
    return z, t, m_of_t(t)


@pytest.mark.parametrize("d", [3, 5])
def test_sparse_cvi_bernoulli_site_update(amd, rng, d):
    """The same for SparseCVIGaussianProcess: the targets summed into the sites of the inducing intervals through p(f_i | pair)."""
    import torch
    from vidp_amd.conditionals import conditional_statistics
    from vidp_amd.likelihoods import Bernoulli
    from vidp_amd.sparse_variational_cvi import SparseCVIGaussianProcess
    from vidp_amd.variational_cvi import back_project_nats
    mk, ok, u, m_np = _step_setup(rng, d)
    z, t, m = _sparse_data(rng, lambda t: 0.2 * t + m_np(t))
    y = ((m + 1.5 * np.sin(3.0 * t) + 0.5 * rng.normal(size=60)) > 0).astype(np.float64)[:, None]
    data = (dev(t), dev(y))
    rho = 0.4
    twin = SparseCVIGaussianProcess(mk(), dev(z), Bernoulli(), learning_rate=rho)
    twin.update_sites(data)
    gk = mk()
    g = SparseCVIGaussianProcess(gk, dev(z), Bernoulli(), mean_function=LinearPlusStep(0.2, _step_mean(gk, u)), learning_rate=rho)
    g.nat1, g.nat2 = twin.nat1.clone(), twin.nat2.clone()
    assert g._data(data) is not None                                       # the fused route
    fmu0, fvar0 = twin.posterior.predict_f(dev(t))
    g1, g2 = _site_targets(Bernoulli(), fmu0, fvar0, dev(m[:, None]), dev(y))
    H = gk.generate_emission_model(dev(t)).emission_matrix
    P, _ = conditional_statistics(dev(t), dev(z), gk)
    b1, b2 = back_project_nats(g1, g2.reshape(g1.shape), H @ P)
    idx = torch.searchsorted(dev(z), dev(t))
    want1 = (1 - rho) * twin.nat1 + rho * torch.zeros_like(twin.nat1).index_add_(0, idx, b1)
    want2 = (1 - rho) * twin.nat2 + rho * torch.zeros_like(twin.nat2).index_add_(0, idx, b2)
    g.update_sites(data)
    np.testing.assert_allclose(host(g.nat1), host(want1), rtol=0, atol=1e-10 * float(want1.abs().max()))
    np.testing.assert_allclose(host(g.nat2), host(want2), rtol=0, atol=1e-10 * float(want2.abs().max()))
    # the generic route (unsorted time points) makes the same step
    perm = rng.permutation(60)
    h = SparseCVIGaussianProcess(gk, dev(z), Bernoulli(), mean_function=LinearPlusStep(0.2, _step_mean(gk, u)), learning_rate=rho)
    h.nat1, h.nat2 = twin.nat1.clone(), twin.nat2.clone()
    shuffled = (dev(t[perm]), dev(y[perm]))
    assert h._data(shuffled) is None
    h.update_sites(shuffled)
    np.testing.assert_allclose(host(h.nat1), host(want1), rtol=0, atol=1e-10 * float(want1.abs().max()))
    np.testing.assert_allclose(host(h.nat2), host(want2), rtol=0, atol=1e-10 * float(want2.abs().max()))
    np.testing.assert_allclose(float(h.classic_elbo(shuffled)), float(g.classic_elbo(data)), rtol=1e-10)


@pytest.mark.parametrize("d", [3, 5])
def test_sparse_cvi_gaussian_equals_the_model_of_the_residuals(amd, rng, d):
    """SparseCVIGaussianProcess(Gaussian) with a mean on y against the mean-free model on y - m: nat1, nat2 and classic_elbo agree to
    1e-10 over three steps; at equal sites posterior.predict_f differs by exactly m."""
    import torch
    from vidp_amd.likelihoods import Gaussian
    from vidp_amd.sparse_variational_cvi import SparseCVIGaussianProcess
    mk, ok, u, m_np = _step_setup(rng, d)
    z, t, _ = _sparse_data(rng, m_np)
    gk = mk()
    mean = _step_mean(gk, u)
    m = mean(dev(t))
    y = dev((m_np(t) + np.sin(2.0 * t) + 0.3 * rng.normal(size=60))[:, None])
    g = SparseCVIGaussianProcess(gk, dev(z), Gaussian(NOISE), mean_function=mean, learning_rate=0.7)
    f = SparseCVIGaussianProcess(mk(), dev(z), Gaussian(NOISE), learning_rate=0.7)
    for _ in range(3):
        g.update_sites((dev(t), y))
        f.update_sites((dev(t), y - m))
        np.testing.assert_allclose(host(g.nat1), host(f.nat1), rtol=0, atol=1e-10 * float(f.nat1.abs().max()))
        np.testing.assert_allclose(host(g.nat2), host(f.nat2), rtol=0, atol=1e-10 * float(f.nat2.abs().max()))
        np.testing.assert_allclose(float(g.classic_elbo((dev(t), y))), float(f.classic_elbo((dev(t), y - m))), rtol=1e-10)
    g.nat1, g.nat2 = f.nat1.clone(), f.nat2.clone()
    tn = dev(np.sort(rng.uniform(-0.5, 9.0, size=15)))
    (gm, gv), (fm, fv) = g.posterior.predict_f(tn), f.posterior.predict_f(tn)
    assert torch.equal(gm, fm + mean(tn)) and torch.equal(gv, fv)
    assert float(mean(tn).abs().max()) > 0.1
    with pytest.raises(NotImplementedError, match="mean function"):
        g.elbo_and_grad((dev(t), y))


def test_sparse_cvi_refuses_a_shared_chain_with_a_mean(amd):
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Gaussian
    from vidp_amd.mean_function import LinearMeanFunction
    from vidp_amd.sparse_variational_cvi import SparseCVIGaussianProcess
    k = K.Sum([K.Matern52(1.0, 1.0), K.Matern52(2.0, 1.0), K.Matern52(3.0, 1.0)])
    with pytest.raises(NotImplementedError, match="shard"):
        SparseCVIGaussianProcess(k, dev(np.arange(8.0)), Gaussian(1.0), mean_function=LinearMeanFunction(1.0), shard=(0, 2))


def test_cvi_step_graph_with_a_mean(amd, rng):
    """step_graph() of CVIGaussianProcess(Bernoulli) with a step mean: three replays give the ELBOs and sites of three eager
    `update_sites(); elbo()` bit for bit (the eager reference on the captured order, as tests/test_gpu_lik.py holds the mean-free
    graph to): the shift is one add of a resident tensor inside the capture."""
    from vidp_amd.likelihoods import Bernoulli
    from vidp_amd.variational_cvi import CVIGaussianProcess
    mk, ok, u, m_np = _step_setup(rng, 3)
    t = _grid40(rng)
    y = ((m_np(t) + 1.5 * np.sin(3.0 * t) + 0.5 * rng.normal(size=40)) > 0).astype(np.float64)[:, None]

    def new():
        k = mk()
        return CVIGaussianProcess((dev(t), dev(y)), k, Bernoulli(), mean_function=_step_mean(k, u), learning_rate=0.5)
    a, b = new(), new()
    step = b.step_graph()
    want, got = [], []
    for _ in range(3):
        a.dist_p.plan.epoch += 1
        a.update_sites()
        want.append(float(a.elbo()))
        got.append(float(step()))
    b.dist_p.plan.check_info()
    assert np.all(np.isfinite(want))
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(host(b.sites.nat1), host(a.sites.nat1))
    np.testing.assert_array_equal(host(b.sites.nat2), host(a.sites.nat2))


def test_kernel_changed_drops_the_cached_mean(amd, rng):
    """After kernel.assign_hyperparameters(...) and kernel_changed() the mean at the data is that of the new kernel."""
    import torch
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Gaussian
    from vidp_amd.sparse_variational_cvi import SparseCVIGaussianProcess
    from vidp_amd.variational_cvi import CVIGaussianProcess
    u = rng.normal(size=(5, 3))
    t = _grid40(rng)
    y = rng.normal(size=(40, 1))
    k = K.Matern52(0.9, 1.2)
    c = CVIGaussianProcess((dev(t), dev(y)), k, Gaussian(NOISE), mean_function=_step_mean(k, u))
    s = SparseCVIGaussianProcess(k, dev(np.linspace(0.3, 7.7, 12)), Gaussian(NOISE), mean_function=_step_mean(k, u))
    old = c._mean_at_data().clone()
    old_s = s._predict_f_data(s._data((dev(t), dev(y))))[0].clone()
    assert c._mean_at_data() is c._mean_at_data()                            # resident
    k.assign_hyperparameters({"lengthscale": 1.7, "variance": 1.2})
    c.kernel_changed()
    s.kernel_changed()
    fresh = _step_mean(K.Matern52(1.7, 1.2), u)(dev(t))
    assert torch.equal(c._mean_at_data(), fresh) and not torch.equal(fresh, old)
    assert torch.equal(s._predict_f_data(s._data((dev(t), dev(y))))[0], fresh)          # zero sites: the prediction is the mean
    assert not torch.equal(old_s, fresh)


# update_sites(); classic_elbo() of the models without a mean function, and GaussianProcessRegression.log_likelihood(), as the commit
# before the mean functions gave them on this data (float.hex, recorded there with the same seed)
RECORDED = {
    "gpr": "-0x1.0e192b1a2aa9cp+5",
    "cvi": "-0x1.b1bceafc89414p+4",
    "sparse": "-0x1.1a6681a6e9c78p+5",
}


def _recorded_values():
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Bernoulli
    from vidp_amd.sparse_variational_cvi import SparseCVIGaussianProcess
    from vidp_amd.variational_cvi import CVIGaussianProcess, GaussianProcessRegression
    rng = np.random.default_rng(2024)
    t = np.sort(rng.uniform(0.0, 8.0, size=60))
    yb = ((1.5 * np.sin(3.0 * t) + 0.5 * rng.normal(size=60)) > 0).astype(np.float64)[:, None]
    tg = _grid40(rng)
    ybg = ((1.5 * np.sin(3.0 * tg) + 0.5 * rng.normal(size=40)) > 0).astype(np.float64)[:, None]
    yg = (np.sin(2.0 * tg) + 0.3 * rng.normal(size=40))[:, None]
    out = {}
    out["gpr"] = float(GaussianProcessRegression((dev(tg), dev(yg)), K.Matern52(0.9, 1.2),
                                                 chol_obs_covariance=dev(np.array([[np.sqrt(NOISE)]]))).log_likelihood()).hex()
    c = CVIGaussianProcess((dev(tg), dev(ybg)), K.Matern52(0.9, 1.2), Bernoulli(), learning_rate=0.5)
    c.update_sites()
    out["cvi"] = float(c.classic_elbo()).hex()
    s = SparseCVIGaussianProcess(K.Matern52(0.9, 1.2), dev(np.linspace(0.3, 7.7, 12)), Bernoulli(), learning_rate=0.5)
    s.update_sites((dev(t), dev(yb)))
    out["sparse"] = float(s.classic_elbo((dev(t), dev(yb)))).hex()
    return out


def test_without_a_mean_function_nothing_changes(amd):
    """mean_function=None: the three models give, bit for bit, the values recorded on the commit before the mean functions (RECORDED),
    and predict_f_at_data hands back the tensors of the zero-mean prediction themselves (no add, no copy)."""
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Bernoulli
    from vidp_amd.variational_cvi import CVIGaussianProcess
    assert _recorded_values() == RECORDED
    t = np.linspace(0.0, 4.0, 30)
    c = CVIGaussianProcess((dev(t), dev((np.sin(t) > 0).astype(np.float64)[:, None])), K.Matern32(1.0, 1.0), Bernoulli())
    seen = []
    inner = c._predict_g_at_data
    c._predict_g_at_data = lambda: seen.append(inner()) or seen[-1]
    out = c.predict_f_at_data()
    assert out[0] is seen[0][0] and out[1] is seen[0][1] and c._mean_at_data() is None
