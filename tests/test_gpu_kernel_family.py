"""
GPU tests of the seasonal kernels (HarmonicOscillator, Constant, Product; kernel k_kernel_ssm, csrc/mfgm_kernel_ssm.h, entry point
mfgm_packed_kernel_ssm): the packed SSM against the NumPy restatement tests/np_kernels_ext.py for d = 1..8, a Matern-only tree through
both entry points, the not-positive-definite report, the GPR log marginal likelihood and the predictive against the dense GP, CVI-GP
(Bernoulli) and sparse CVI (Poisson) against the oracle models, seeded sampling and the hyper-parameter tape.  fp64.
"""
import numpy as np
import pytest

from oracle import np_kernels, np_models
from tests import np_kernels_ext as E
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


def tree(name, m, x, jitter=0.0):
    """The named test kernel built from the Matern module m and the seasonal module x (vidp_amd.kernels twice, or np_kernels and
    np_kernels_ext)."""
    P, S, HO, C = x.Product, m.Sum, x.HarmonicOscillator, x.Constant
    k = {
        "c": lambda: C(1.7),
        "ho": lambda: HO(1.3, 0.8),
        "m52c": lambda: P([m.Matern52(0.9, 1.1), C(0.6)]),
        "m32ho": lambda: P([m.Matern32(0.7, 1.3), HO(1.0, 1.5)]),
        "m52_m12ho": lambda: S([m.Matern52(0.5, 1.0), P([m.Matern12(0.8, 2.0), HO(0.7, 0.6)])]),
        "m52ho": lambda: P([m.Matern52(1.2, 0.9), HO(1.0, 2.5)]),
        "m32m52": lambda: P([m.Matern32(0.9, 1.2), m.Matern52(1.4, 0.7)]),
        "m32ho_m52": lambda: S([P([m.Matern32(0.4, 0.5), HO(1.0, 1.1)]), m.Matern52(2.0, 1.5)]),
        "hom32ho": lambda: P([HO(1.0, 3.0), m.Matern32(1.5, 0.8), HO(0.5, 0.7)]),
        "m12cho_c": lambda: S([P([m.Matern12(0.6, 1.0), C(2.0), HO(0.8, 1.3)]), P([C(0.4), m.Matern52(0.7, 0.5)]), m.Matern52(0.3, 0.2)]),
        "d12": lambda: S([P([m.Matern52(1.2, 0.9), HO(1.0, 2.5)]), P([m.Matern52(0.4, 0.3), HO(0.5, 0.9)])]),
        "sum_x_ho": lambda: P([S([m.Matern12(0.5, 1.0), m.Matern32(1.0, 0.5)]), HO(1.0, 1.7)]),
    }[name]()
    k.jitter = jitter
    return k


def set_means(gk, ok, rng):
    """The same random state mean on both trees (on the children of a Sum, whose mean is theirs)."""
    if hasattr(gk, "kernels") and type(gk).__name__ == "Sum":
        for g, o in zip(gk.kernels, ok.kernels):
            set_means(g, o, rng)
        return
    m = rng.normal(size=gk.state_dim)
    gk.set_state_mean(m)
    ok._state_mean = m


D_CASES = [("c", 1), ("ho", 2), ("m52c", 3), ("m32ho", 4), ("m52_m12ho", 5), ("m52ho", 6), ("m32m52", 6), ("m32ho_m52", 7),
           ("hom32ho", 8), ("m12cho_c", 8)]


@pytest.mark.parametrize("name,d", D_CASES)
@pytest.mark.parametrize("jitter", [0.0, 1e-6])
def test_kernel_ssm_matches_numpy(amd, rng, name, d, jitter, batch_shape):
    """mfgm_packed_kernel_ssm against np_kernels_ext: A, b, chol Q chol Q^T and the initial moments within 1e-12 of max |Pinf| (A within
    1e-12 of its own scale), on gaps 0, O(0.3) and many periods (tiny gaps 1e-7 with the jitter), with the default partition and with
    5-node segments (every segment boundary takes the transition into the segment's first node)."""
    from vidp_amd import kernels as K
    from vidp_amd.packed import Plan
    gk, ok = tree(name, K, K, jitter), tree(name, np_kernels, E, jitter)
    assert gk.state_dim == ok.state_dim == d
    set_means(gk, ok, rng)
    gaps = [0.0, 0.3, 17.3, 0.0, 41.0] + ([1e-7, 1e-7] if jitter else [0.2, 0.1])
    dt = np.concatenate([rng.exponential(0.3, size=batch_shape + (20,)), np.broadcast_to(gaps, batch_shape + (len(gaps),))], axis=-1)
    dt = np.take_along_axis(dt, np.argsort(rng.uniform(size=dt.shape), axis=-1), axis=-1)
    t = np.concatenate([np.zeros(batch_shape + (1,)), np.cumsum(dt, axis=-1)], axis=-1)
    oA, oQ = ok.transition_statistics(np.diff(t, axis=-1))
    ob = ok.state_offsets(np.diff(t, axis=-1))
    Pinf = ok.steady_state_covariance()
    scale = np.abs(Pinf).max()
    B = int(np.prod(batch_shape))
    for plan in (None, Plan(B, t.shape[-1], d, R0=5, device="cuda")):
        g = gk.state_space_model(dev(t), plan=plan)
        np.testing.assert_allclose(host(g.state_transitions), oA, rtol=0, atol=1e-12 * max(1.0, np.abs(oA).max()))
        np.testing.assert_allclose(host(g.state_offsets), ob, rtol=0, atol=1e-12 * max(1.0, np.abs(ob).max()))
        c = host(g.cholesky_process_covariances)
        np.testing.assert_allclose(c @ np.swapaxes(c, -1, -2), oQ, rtol=0, atol=1e-12 * scale)
        c0 = host(g.cholesky_initial_covariance)
        np.testing.assert_allclose(c0 @ np.swapaxes(c0, -1, -2), np.broadcast_to(ok.initial_covariance(), c0.shape), rtol=0,
                                   atol=1e-12 * scale)
        np.testing.assert_allclose(host(g.initial_mean), np.broadcast_to(ok.state_mean, batch_shape + (d,)), rtol=0, atol=1e-15)
        if jitter == 0.0 and name in ("c", "ho"):
            assert (c == 0).all()                      # cholesky_or_zero: the noise-free kernels' Q is exactly zero
    H = host(gk.generate_emission_model(dev(t)).emission_matrix)
    np.testing.assert_array_equal(H, ok.emission_matrix(t))


def test_matern_tree_through_both_entry_points(amd, rng):
    """A Matern-only tree through mfgm_packed_kernel_ssm and through mfgm_packed_stationary_ssm: equal within 1e-12 of max |Pinf|
    (tools/kernel_rate.py reports whether they are bit-identical)."""
    from vidp_amd import kernels as K
    from vidp_amd.packed import Plan
    k = K.Sum([K.Matern52(0.5, 1.0), K.Matern32(1.5, 0.3), K.Matern12(0.8, 2.0), K.OrnsteinUhlenbeck(1.2, 0.4)], jitter=1e-9)
    k.kernels[0].set_state_mean(rng.normal(size=3))
    t = np.cumsum(np.concatenate([[0.0, 0.0], rng.exponential(0.2, size=(300,)), [25.0]]))[None].repeat(3, axis=0)
    B, T = t.shape
    plan = Plan(B, T, k.state_dim, R0=7, device="cuda")
    dts = (dev(t)[:, 1:] - dev(t)[:, :-1]).contiguous()
    a = unpacked(plan, plan.stationary_ssm(k._spec(), dts))
    b = unpacked(plan, plan.kernel_ssm(k._terms_struct(), dts))
    plan.check_info()
    scale = float(k.steady_state_covariance.abs().max())
    for x, y in zip(a, b):
        np.testing.assert_allclose(host(y), host(x), rtol=0, atol=1e-12 * scale)


def unpacked(plan, packed):
    """(A [B, T-1, d, d], off [B, T, d], chol [B, T, d, d]) from the packed arrays (the padding of the packed layout is never written)."""
    from vidp_amd._lib import FULL, TRI, VEC
    A, off, chol = packed
    return plan.unpack(FULL, A, plan.T - 1), plan.unpack(VEC, off), plan.unpack(TRI, chol)


def test_not_positive_definite_q_raises(amd):
    """Sum(Matern12, HarmonicOscillator) with no jitter: Q = diag(q, 0, 0) is neither positive definite nor zero."""
    from vidp_amd import kernels as K
    t = dev(np.linspace(0.0, 3.0, 30))
    k = K.Sum([K.Matern12(1.0, 1.0), K.HarmonicOscillator(1.0, 1.0)])
    with pytest.raises(ArithmeticError, match="set a jitter"):
        k.state_space_model(t)
    k.jitter = 1e-6
    k.state_space_model(t)
    # a jitter on a child of a Sum still raises
    with pytest.raises(ValueError, match="per-component jitter"):
        K.Sum([K.Matern12(1.0, 1.0), K.HarmonicOscillator(1.0, 1.0, jitter=1e-6)]).state_space_model(t)


def _dense_logml(ok, t, y, noise):
    Kd = E.dense_k(ok, t[:, None] - t[None, :]) + noise * np.eye(t.size)
    L = np.linalg.cholesky(Kd)
    a = np.linalg.solve(L, y[:, 0])
    return -0.5 * a @ a - np.log(np.diag(L)).sum() - 0.5 * t.size * np.log(2 * np.pi)


@pytest.mark.parametrize("name", ["m32ho", "m52_m12ho", "d12"])
def test_gpr_log_likelihood_equals_the_dense_gp(amd, rng, name):
    """GaussianProcessRegression.log_likelihood() (Kalman filter over the kernel's SSM; d = 12 through the torch closed forms and the
    wide sweeps) equals the dense GP log marginal likelihood (NumPy Cholesky of the 400 x 400 Gram matrix) at rtol 1e-9."""
    from vidp_amd import kernels as K
    from vidp_amd.variational_cvi import GaussianProcessRegression
    gk, ok = tree(name, K, K), tree(name, np_kernels, E)
    # gaps >= 0.03: Q = Pinf - A Pinf A^T of a Matern factor loses digits to cancellation at tiny gaps, in any SSM
    t = np.linspace(0.0, 20.0, 400) + rng.uniform(-0.01, 0.01, size=400)
    y = np.sin(2.0 * t)[:, None] + 0.3 * rng.normal(size=(400, 1))
    noise = 0.2
    g = GaussianProcessRegression((dev(t), dev(y)), gk, chol_obs_covariance=dev(np.array([[np.sqrt(noise)]])))
    np.testing.assert_allclose(float(g.log_likelihood()), _dense_logml(ok, t, y, noise), rtol=1e-9)
    np.testing.assert_allclose(float(g.log_likelihood()), np_models.gpr_log_likelihood(t, y, ok, noise), rtol=1e-9)


def test_gpr_predictive_and_sampling(amd, rng):
    """AnalyticPosteriorProcess.predict_f at new, unsorted times equals the dense GP predictive (1e-8); sample_f is reproducible."""
    from vidp_amd import kernels as K
    from vidp_amd.variational_cvi import GaussianProcessRegression
    name = "m32ho"
    gk, ok = tree(name, K, K), tree(name, np_kernels, E)
    t = np.linspace(0.0, 8.0, 120) + rng.uniform(-0.01, 0.01, size=120)
    y = np.cos(1.5 * t)[:, None] + 0.2 * rng.normal(size=(120, 1))
    noise = 0.1
    g = GaussianProcessRegression((dev(t), dev(y)), gk, chol_obs_covariance=dev(np.array([[np.sqrt(noise)]])))
    tn = rng.uniform(-1.0, 9.0, size=37)
    mu, var = g.posterior.predict_f(dev(tn))
    Kd = E.dense_k(ok, t[:, None] - t[None, :]) + noise * np.eye(t.size)
    Ks = E.dense_k(ok, tn[:, None] - t[None, :])
    om = Ks @ np.linalg.solve(Kd, y[:, 0])
    ov = E.dense_k(ok, np.zeros(tn.size)) - np.einsum("ij,ji->i", Ks, np.linalg.solve(Kd, Ks.T))
    np.testing.assert_allclose(host(mu).reshape(-1), om, rtol=1e-8, atol=1e-8)
    np.testing.assert_allclose(host(var).reshape(-1), ov, rtol=1e-8, atol=1e-8)
    s1 = host(g.posterior.sample_f(dev(tn), (4,), seed=11))
    s2 = host(g.posterior.sample_f(dev(tn), (4,), seed=11))
    s3 = host(g.posterior.sample_f(dev(tn), (4,), seed=12))
    np.testing.assert_array_equal(s1, s2)
    assert np.isfinite(s1).all() and not np.array_equal(s1, s3)


def _cls_data(rng, n, which, t):
    f = 1.5 * np.sin(3 * t)
    if which == "bernoulli":
        y = (f + 0.5 * rng.normal(size=n) > 0).astype(np.float64)
    else:
        y = rng.poisson(np.exp(f)).astype(np.float64)
    return t, y[:, None]


def test_cvi_gp_bernoulli_against_oracle(amd, rng):
    """CVIGaussianProcess with a Bernoulli likelihood on the quasi-periodic prior Product(Matern32, HarmonicOscillator) follows
    oracle/np_models.CVIGaussianProcess with the ext kernels for 8 damped steps (the tolerances of tests/test_gpu_lik.py)."""
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Bernoulli
    from vidp_amd.variational_cvi import CVIGaussianProcess
    t, y = _cls_data(rng, 30, "bernoulli", np.linspace(0.0, 4.0, 30))
    g = CVIGaussianProcess((dev(t), dev(y)), tree("m32ho", K, K), Bernoulli(), learning_rate=0.5)
    o = np_models.CVIGaussianProcess(t, y, tree("m32ho", np_kernels, E), np_lik.Bernoulli(), learning_rate=0.5)
    for _ in range(8):
        g.update_sites()
        o.update_sites()
        np.testing.assert_allclose(host(g.sites.nat1), o.nat1, rtol=1e-9, atol=1e-9 * np.abs(o.nat1).max())
        np.testing.assert_allclose(host(g.sites.nat2), o.nat2, rtol=1e-9, atol=1e-9 * np.abs(o.nat2).max())
        np.testing.assert_allclose(float(g.elbo()), o.elbo(), rtol=1e-9)
        np.testing.assert_allclose(float(g.classic_elbo()), o.classic_elbo(), rtol=1e-9)


@pytest.mark.parametrize("route", ["fused", "generic"])
def test_sparse_cvi_poisson_against_oracle(amd, rng, monkeypatch, route):
    """SparseCVIGaussianProcess with a Poisson likelihood on Product(Matern52, HarmonicOscillator) (d = 6) follows
    oracle/np_conditionals.SparseCVIGaussianProcess for 5 steps, on the fused sorted-data route and on the generic route."""
    from oracle import np_conditionals as npc
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Poisson
    from vidp_amd.sparse_variational_cvi import SparseCVIGaussianProcess
    if route == "generic":
        monkeypatch.setenv("VIDP_FUSED_SPARSE", "0")
    t, y = _cls_data(rng, 40, "poisson", np.linspace(0.0, 1.0, 40))
    z = np.linspace(-0.1, 1.1, 9)
    mk = lambda m, x: x.Product([m.Matern52(0.6, 1.2), x.HarmonicOscillator(1.0, 0.7)], jitter=1e-9)
    g = SparseCVIGaussianProcess(mk(K, K), dev(z), Poisson(1.3), learning_rate=0.6)
    o = npc.SparseCVIGaussianProcess(mk(np_kernels, E), z, np_lik.Poisson(1.3), learning_rate=0.6)
    data = (dev(t), dev(y))
    assert (g._data(data) is None) == (route == "generic")
    for _ in range(5):
        g.update_sites(data)
        o.update_sites(t, y)
        np.testing.assert_allclose(host(g.nat1), o.nat1, rtol=1e-9, atol=1e-9 * np.abs(o.nat1).max())
        np.testing.assert_allclose(host(g.nat2), o.nat2, rtol=1e-9, atol=1e-9 * np.abs(o.nat2).max())
        np.testing.assert_allclose(float(g.classic_elbo(data)), o.classic_elbo(t, y), rtol=1e-9)


def test_classic_elbo_tape_hyper_learns_the_period(amd, rng):
    """d classic_elbo / d (period, variance) of the oscillator and d / d (lengthscale, variance) of the Matern factor through the tape
    agree with a fourth-order difference quotient of the same ELBO (with a Gaussian likelihood the optimal sites do not depend on the
    kernel, so the ELBO at them is the GPR log marginal likelihood of every hyper-parameter value) at rtol 1e-6."""
    import torch
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Gaussian
    from vidp_amd.variational_cvi import CVIGaussianProcess
    hyp = [[0.9, 1.1], [0.8, 1.7]]          # Matern32 (lengthscale, variance), oscillator (variance, period)

    def mk(m, x, h):
        return x.Product([m.Matern32(*h[0]), x.HarmonicOscillator(*h[1])])
    t = np.linspace(0.0, 5.0, 12) + 0.05 * rng.uniform(-1, 1, size=12)
    y = np.sin(2 * t)[:, None] + 0.1 * rng.normal(size=(12, 1))
    noise = 0.4
    g = CVIGaussianProcess((dev(t), dev(y)), mk(K, K, hyp), Gaussian(noise), learning_rate=1.0)
    g.update_sites()
    elbo, leaves = g.classic_elbo_tape_hyper()
    ref = lambda h: np_models.gpr_log_likelihood(t, y, mk(np_kernels, E, h), noise)
    np.testing.assert_allclose(float(elbo.detach()), ref(hyp), rtol=1e-8)
    names = [(0, "lengthscale", 0), (0, "variance", 1), (1, "variance", 0), (1, "period", 1)]
    grads = torch.autograd.grad(elbo, [leaves[c][n] for c, n, _ in names])
    for (c, n, i), gr in zip(names, grads):
        def at(e):
            h = [list(x) for x in hyp]
            h[c][i] += e
            return ref(h)
        e = 1e-3
        fd = (8 * (at(e) - at(-e)) - (at(2 * e) - at(-2 * e))) / (12 * e)
        np.testing.assert_allclose(float(gr), fd, rtol=1e-6, atol=1e-8)
