"""
GPU tests of the latent exponentially generated kernel (vidp_amd.kernels.LatentExponentiallyGenerated; kernels k_leg_ssm and
k_leg_transitions, csrc/mfgm_leg_ssm.h; entry points mfgm_packed_leg_ssm and mfgm_leg_transitions): the packed SSM against the
NumPy restatement tests/np_leg.py for d = 1..8, its edges, the natural-layout transitions, a closed-form twin (damped cosine), the
dependence of a transition on its gap alone, the models and the hyper-parameter tape.  fp64.
"""
import numpy as np
import pytest

from oracle import np_kernels, np_models
from tests import np_kernels_ext as E
from tests import np_leg as L
from tests import np_lik

pytestmark = pytest.mark.gpu

EXTRA_GAPS = [0.0, 0.3, 17.3, 0.0, 41.0, 1e-3, 0.1]


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


def pair(N, R, jitter=0.0, emission=None):
    """The kernel and its NumPy restatement."""
    from vidp_amd import kernels as K
    return K.LatentExponentiallyGenerated(N, R, jitter=jitter, emission=emission), L.LatentExponentiallyGenerated(N, R, jitter, emission)


@pytest.mark.parametrize("d", range(1, 9))
@pytest.mark.parametrize("jitter", [0.0, 1e-6])
def test_leg_ssm_matches_numpy(amd, rng, d, jitter, batch_shape):
    """mfgm_packed_leg_ssm against np_leg (long-double exponential): A, b, chol Q chol Q^T and the initial covariance within
    1e-12 max(1, scale), the initial mean within 1e-15, on 20 gaps ~ Exp(0.3) plus 0, 1e-3, 0.1, 0.3, 17.3, 41 shuffled, with the
    default partition and with 5-node segments; at the zero gaps A == I and chol == 0 exactly when there is no jitter.  The Cholesky
    comparison is well-posed: lambda_min(Q) >= 1e-6 at every non-zero gap, asserted from the oracle."""
    from vidp_amd.packed import Plan
    N, R = rng.random((d, d)) + np.eye(d), rng.random((d, d))
    gk, ok = pair(N, R, jitter)
    m = rng.normal(size=d)
    gk.set_state_mean(m)
    ok._state_mean = m
    dt = np.concatenate([rng.exponential(0.3, size=batch_shape + (20,)), np.broadcast_to(EXTRA_GAPS, batch_shape + (len(EXTRA_GAPS),))],
                        axis=-1)
    dt = np.take_along_axis(dt, np.argsort(rng.uniform(size=dt.shape), axis=-1), axis=-1)
    t = np.concatenate([np.zeros(batch_shape + (1,)), np.cumsum(dt, axis=-1)], axis=-1)
    gaps = np.diff(t, axis=-1)
    oA, oQ = ok.transition_statistics(gaps)
    ob = ok.state_offsets(gaps)
    lam_min = np.linalg.eigvalsh(oQ)[..., 0][gaps > 0].min()
    print(f"d={d} jitter={jitter} lambda_min(Q) over the non-zero gaps = {lam_min:.3e}")
    assert lam_min >= 1e-6
    B = int(np.prod(batch_shape))
    eye = np.eye(d)
    for plan in (None, Plan(B, t.shape[-1], d, R0=5, device="cuda")):
        g = gk.state_space_model(dev(t), plan=plan)
        gA, gb, c = host(g.state_transitions), host(g.state_offsets), host(g.cholesky_process_covariances)
        c0 = host(g.cholesky_initial_covariance)
        print(f"  max|A - oA|={np.abs(gA - oA).max():.3e} max|b - ob|={np.abs(gb - ob).max():.3e} "
              f"max|cc^T - oQ|={np.abs(c @ np.swapaxes(c, -1, -2) - oQ).max():.3e}")
        np.testing.assert_allclose(gA, oA, rtol=0, atol=1e-12 * max(1.0, np.abs(oA).max()))
        np.testing.assert_allclose(gb, ob, rtol=0, atol=1e-12 * max(1.0, np.abs(ob).max()))
        np.testing.assert_allclose(c @ np.swapaxes(c, -1, -2), oQ, rtol=0, atol=1e-12)
        np.testing.assert_allclose(c0 @ np.swapaxes(c0, -1, -2), np.broadcast_to(ok.initial_covariance(), c0.shape), rtol=0, atol=1e-12)
        np.testing.assert_allclose(host(g.initial_mean), np.broadcast_to(m, batch_shape + (d,)), rtol=0, atol=1e-15)
        if jitter == 0.0:
            assert (gaps == 0).sum() == 2 * B
            np.testing.assert_array_equal(gA[gaps == 0], np.broadcast_to(eye, (2 * B, d, d)))
            assert (c[gaps == 0] == 0).all()
    H = host(gk.generate_emission_model(dev(t)).emission_matrix)
    np.testing.assert_array_equal(H, ok.emission_matrix(t))


@pytest.mark.parametrize("T", [1, 2])
def test_shortest_chains(amd, rng, T):
    """T = 1 (no transition: mfgm_packed_leg_ssm takes a null time_deltas and writes node 0 only) and T = 2 chains, on the packed
    arrays."""
    from vidp_amd._lib import FULL, TRI, VEC
    from vidp_amd.packed import Plan
    d = 3
    gk, ok = pair(rng.random((d, d)) + np.eye(d), rng.random((d, d)), 1e-6)
    m = rng.normal(size=d)
    gk.set_state_mean(m)
    ok._state_mean = m
    gaps = rng.exponential(0.5, size=(2, T - 1))
    plan = Plan(2, T, d, device="cuda")
    A, off, chol = plan.leg_ssm(gk._spec(), dev(gaps) if T > 1 else None)
    plan.check_info()
    off, c = host(plan.unpack(VEC, off)), host(plan.unpack(TRI, chol))
    np.testing.assert_allclose(c[:, 0] @ np.swapaxes(c[:, 0], -1, -2), np.broadcast_to((1.0 + 1e-6) * np.eye(d), (2, d, d)), rtol=0,
                               atol=1e-12)
    np.testing.assert_allclose(off[:, 0], np.broadcast_to(m, (2, d)), rtol=0, atol=1e-15)
    if T == 2:
        oA, oQ = ok.transition_statistics(gaps)
        np.testing.assert_allclose(host(plan.unpack(FULL, A, 1)), oA, rtol=0, atol=1e-12)
        np.testing.assert_allclose(c[:, 1:] @ np.swapaxes(c[:, 1:], -1, -2), oQ, rtol=0, atol=1e-12)
        np.testing.assert_allclose(off[:, 1:], ok.state_offsets(gaps), rtol=0, atol=1e-12 * max(1.0, np.abs(m).max()))
        g = gk.state_space_model(dev(np.concatenate([np.zeros((2, 1)), gaps], axis=-1)))
        np.testing.assert_array_equal(host(g.state_transitions), host(plan.unpack(FULL, A, 1)))


def test_pure_rotation(amd, rng):
    """N = 0 with no jitter is a pure rotation, Q = I - A A^T = 0 up to rounding.  The contract allows two outcomes: every Q exactly
    zero (chol == 0) or the "set a jitter" ArithmeticError.  Observed on the MI355X: it raises -- the rounding leaves entries of order
    1e-16 in Q, which is then neither zero nor positive definite.  With jitter = 1e-9 the same kernel builds."""
    R = np.array([[0.0, 1.7], [0.0, 0.0]])
    t = np.cumsum(np.concatenate([[0.0], rng.exponential(0.4, size=24)]))
    gk, ok = pair(np.zeros((2, 2)), R)
    try:
        g = gk.state_space_model(dev(t))
    except ArithmeticError as e:
        outcome = "raises"
        assert "set a jitter" in str(e)
    else:
        outcome = "zero"
        assert (host(g.cholesky_process_covariances) == 0).all()
    print("pure rotation without jitter:", outcome)
    gk, ok = pair(np.zeros((2, 2)), R, 1e-9)
    g = gk.state_space_model(dev(t))
    oA, oQ = ok.transition_statistics(np.diff(t))
    c = host(g.cholesky_process_covariances)
    np.testing.assert_allclose(host(g.state_transitions), oA, rtol=0, atol=1e-12)
    np.testing.assert_allclose(c @ np.swapaxes(c, -1, -2), oQ, rtol=0, atol=1e-12)


@pytest.mark.parametrize("d", [1, 3, 8])
def test_leg_transitions_match_numpy(amd, rng, d):
    """mfgm_leg_transitions on unordered gaps [7, 3] including 0 (and on a single gap) against np_leg to 1e-12; A agrees bit for bit
    with the packed build's, Q is symmetric and carries the jitter."""
    gk, ok = pair(rng.random((d, d)) + np.eye(d), rng.random((d, d)), 1e-6)
    dt = rng.exponential(0.5, size=(7, 3))
    dt[2, 1], dt[5, 0], dt[0, 2] = 0.0, 23.0, 1e-4
    A, Q = gk.transition_statistics_local(dev(dt))
    oA, oQ = ok.transition_statistics(dt)
    assert tuple(A.shape) == tuple(Q.shape) == (7, 3, d, d)
    np.testing.assert_allclose(host(A), oA, rtol=0, atol=1e-12)
    np.testing.assert_allclose(host(Q), oQ, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(host(Q), np.swapaxes(host(Q), -1, -2))
    np.testing.assert_array_equal(host(A)[2, 1], np.eye(d))
    np.testing.assert_array_equal(host(Q)[2, 1], 1e-6 * np.eye(d))
    A1, Q1 = gk.transition_statistics_local(dev(dt[3:4, 1]))
    np.testing.assert_array_equal(host(A1)[0], host(A)[3, 1])
    np.testing.assert_array_equal(host(Q1)[0], host(Q)[3, 1])
    A0, Q0 = gk.transition_statistics_local(dev(np.zeros((0,))))
    assert tuple(A0.shape) == (0, d, d)
    # the same exponential as the packed build
    from vidp_amd._lib import FULL
    from vidp_amd.packed import Plan
    plan = Plan(1, dt.size + 1, d, device="cuda")
    Ap, _, _ = plan.leg_ssm(gk._spec(), dev(dt.reshape(1, -1)))
    plan.check_info()
    np.testing.assert_array_equal(host(plan.unpack(FULL, Ap, dt.size))[0], host(A).reshape(-1, d, d))


def _dense_logml(K, y, noise):
    Kd = K + noise * np.eye(y.shape[0])
    c = np.linalg.cholesky(Kd)
    a = np.linalg.solve(c, y[:, 0])
    return -0.5 * a @ a - np.log(np.diag(c)).sum() - 0.5 * y.shape[0] * np.log(2 * np.pi)


def _dense_predict(ok_k, t, y, noise, tn):
    Kd = ok_k(t[:, None] - t[None, :]) + noise * np.eye(t.size)
    Ks = ok_k(tn[:, None] - t[None, :])
    mu = Ks @ np.linalg.solve(Kd, y[:, 0])
    var = ok_k(np.zeros(tn.size)) - np.einsum("ij,ji->i", Ks, np.linalg.solve(Kd, Ks.T))
    return mu, var


def test_damped_cosine_equals_matern12_times_oscillator(amd, rng):
    """LEG with N = sqrt(2 lam) I, R = [[0, omega], [0, 0]] and Product([Matern12(1 / lam, 1), HarmonicOscillator(1, 4 pi / omega)])
    are the same prior, k(tau) = exp(-lam |tau|) cos(omega tau / 2): the same GPR log marginal likelihood and predict_f on T = 40
    irregular points, to 1e-10 relative (vectors: 1e-10 of their largest entry)."""
    from vidp_amd import kernels as K
    from vidp_amd.variational_cvi import GaussianProcessRegression
    lam, omega = 0.7, 2.6
    leg = K.LatentExponentiallyGenerated(np.sqrt(2 * lam) * np.eye(2), np.array([[0.0, omega], [0.0, 0.0]]))
    twin = K.Product([K.Matern12(1.0 / lam, 1.0), K.HarmonicOscillator(1.0, 4.0 * np.pi / omega)])
    t = np.cumsum(rng.exponential(0.25, size=40))
    y = np.cos(1.3 * t)[:, None] + 0.3 * rng.normal(size=(40, 1))
    tn = rng.uniform(t[0] - 0.5, t[-1] + 0.5, size=15)
    chol_noise = dev(np.array([[np.sqrt(0.1)]]))
    out = []
    for k in (leg, twin):
        g = GaussianProcessRegression((dev(t), dev(y)), k, chol_obs_covariance=chol_noise)
        mu, var = g.posterior.predict_f(dev(tn))
        out.append((float(g.log_likelihood()), host(mu).reshape(-1), host(var).reshape(-1)))
    (la, ma, va), (lb, mb, vb) = out
    print(f"logml {la!r} {lb!r} max|dmu|={np.abs(ma - mb).max():.3e} max|dvar|={np.abs(va - vb).max():.3e}")
    np.testing.assert_allclose(la, lb, rtol=1e-10)
    np.testing.assert_allclose(ma, mb, rtol=0, atol=1e-10 * np.abs(mb).max())
    np.testing.assert_allclose(va, vb, rtol=0, atol=1e-10 * np.abs(vb).max())
    # and both are the dense GP with the closed-form covariance
    kf = lambda tau: np.exp(-lam * np.abs(tau)) * np.cos(0.5 * omega * tau)
    np.testing.assert_allclose(la, _dense_logml(kf(t[:, None] - t[None, :]), y, 0.1), rtol=1e-9)


@pytest.mark.parametrize("d", [3, 8])
def test_outputs_depend_on_the_gap_only(amd, rng, d):
    """Chains whose gaps repeat one value: runs of it inside a segment and across 5-node segment boundaries, a run broken by another
    gap, the value after a zero gap and in another chain (dyadic gaps, so the time differences are bit-equal by construction).  Every
    A_k, chol Q_k and b_k of one gap is bit-identical, whatever the lane kept from its previous transition."""
    from vidp_amd.packed import Plan
    gk, _ = pair(rng.random((d, d)) + np.eye(d), rng.random((d, d)), 0.0)
    gk.set_state_mean(rng.normal(size=d))
    d1, d2 = 0.125, 0.5
    chain = [d1] * 4 + [d2] + [d1] * 6 + [0.25, d1, 0.25] + [d1] * 7 + [0.0, d1, 0.0, 0.0, d1, d1]
    dt = np.array([chain, chain[::-1]])
    t = np.concatenate([np.zeros((2, 1)), np.cumsum(dt, axis=-1)], axis=-1)
    np.testing.assert_array_equal(np.diff(t, axis=-1), dt)
    for plan in (None, Plan(2, t.shape[-1], d, R0=5, device="cuda")):
        g = gk.state_space_model(dev(t), plan=plan)
        A, C, b = host(g.state_transitions), host(g.cholesky_process_covariances), host(g.state_offsets)
        for v in (d1, 0.25, 0.0):
            for x in (A[dt == v], C[dt == v], b[dt == v]):
                np.testing.assert_array_equal(x, np.broadcast_to(x[0], x.shape))


def test_gpr_and_predict_f_equal_the_dense_gp(amd, rng):
    """GaussianProcessRegression.log_likelihood() on a d = 3 LEG prior with an emission vector B, T = 30, equals the dense Gaussian log
    density built from k(tau) = B expm(F |tau|) B^T at rtol 1e-9, and predict_f at 15 off-grid, unsorted times equals the dense GP
    predictive (1e-8, the bound of test_gpu_kernel_family.py); sample_f is reproducible."""
    from vidp_amd.variational_cvi import GaussianProcessRegression
    d = 3
    gk, ok = pair(rng.random((d, d)) + np.eye(d), rng.random((d, d)), emission=[1.0, -0.6, 0.4])
    t = np.cumsum(rng.uniform(0.05, 0.4, size=30))
    y = np.sin(2.0 * t)[:, None] + 0.3 * rng.normal(size=(30, 1))
    noise = 0.2
    g = GaussianProcessRegression((dev(t), dev(y)), gk, chol_obs_covariance=dev(np.array([[np.sqrt(noise)]])))
    kf = lambda tau: L.dense_k(ok, tau)
    np.testing.assert_allclose(float(g.log_likelihood()), _dense_logml(kf(t[:, None] - t[None, :]), y, noise), rtol=1e-9)
    np.testing.assert_allclose(float(g.log_likelihood()), np_models.gpr_log_likelihood(t, y, ok, noise), rtol=1e-9)
    tn = rng.uniform(t[0] - 1.0, t[-1] + 1.0, size=15)
    mu, var = g.posterior.predict_f(dev(tn))
    om, ov = _dense_predict(kf, t, y, noise, tn)
    np.testing.assert_allclose(host(mu).reshape(-1), om, rtol=1e-8, atol=1e-8)
    np.testing.assert_allclose(host(var).reshape(-1), ov, rtol=1e-8, atol=1e-8)
    s1 = host(g.posterior.sample_f(dev(tn), (4,), seed=11))
    s2 = host(g.posterior.sample_f(dev(tn), (4,), seed=11))
    np.testing.assert_array_equal(s1, s2)
    assert np.isfinite(s1).all()


def _cls_data(rng, which, t):
    f = 1.5 * np.sin(3 * t)
    if which == "bernoulli":
        y = (f + 0.5 * rng.normal(size=t.size) > 0).astype(np.float64)
    else:
        y = rng.poisson(np.exp(f)).astype(np.float64)
    return y[:, None]


def test_cvi_gp_bernoulli_against_oracle(amd, rng):
    """CVIGaussianProcess with a Bernoulli likelihood on a d = 3 LEG prior follows oracle/np_models.CVIGaussianProcess on np_leg for
    3 damped steps (the tolerances of tests/test_gpu_kernel_family.py)."""
    from vidp_amd.likelihoods import Bernoulli
    from vidp_amd.variational_cvi import CVIGaussianProcess
    gk, ok = pair(rng.random((3, 3)) + np.eye(3), rng.random((3, 3)))
    t = np.linspace(0.0, 4.0, 30)
    y = _cls_data(rng, "bernoulli", t)
    g = CVIGaussianProcess((dev(t), dev(y)), gk, Bernoulli(), learning_rate=0.5)
    o = np_models.CVIGaussianProcess(t, y, ok, np_lik.Bernoulli(), learning_rate=0.5)
    for _ in range(3):
        g.update_sites()
        o.update_sites()
        np.testing.assert_allclose(host(g.sites.nat1), o.nat1, rtol=1e-9, atol=1e-9 * np.abs(o.nat1).max())
        np.testing.assert_allclose(host(g.sites.nat2), o.nat2, rtol=1e-9, atol=1e-9 * np.abs(o.nat2).max())
        np.testing.assert_allclose(float(g.elbo()), o.elbo(), rtol=1e-9)
        np.testing.assert_allclose(float(g.classic_elbo()), o.classic_elbo(), rtol=1e-9)


@pytest.mark.parametrize("route", ["fused", "generic"])
def test_sparse_cvi_poisson_against_oracle(amd, rng, monkeypatch, route):
    """SparseCVIGaussianProcess with a Poisson likelihood on a d = 3 LEG prior, M = 12 inducing points and N = 60 data, follows
    oracle/np_conditionals.SparseCVIGaussianProcess on np_leg for 3 steps, on the fused sorted-data route and on the generic route
    (the conditionals call mfgm_leg_transitions on unordered gaps, the outer ones of 1e10)."""
    from oracle import np_conditionals as npc
    from vidp_amd.likelihoods import Poisson
    from vidp_amd.sparse_variational_cvi import SparseCVIGaussianProcess
    if route == "generic":
        monkeypatch.setenv("VIDP_FUSED_SPARSE", "0")
    gk, ok = pair(rng.random((3, 3)) + np.eye(3), rng.random((3, 3)), 1e-9)
    t = np.linspace(0.0, 1.0, 60)
    y = _cls_data(rng, "poisson", t)
    z = np.linspace(-0.1, 1.1, 12)
    g = SparseCVIGaussianProcess(gk, dev(z), Poisson(1.3), learning_rate=0.6)
    o = npc.SparseCVIGaussianProcess(ok, z, np_lik.Poisson(1.3), learning_rate=0.6)
    data = (dev(t), dev(y))
    assert (g._data(data) is None) == (route == "generic")
    for _ in range(3):
        g.update_sites(data)
        o.update_sites(t, y)
        np.testing.assert_allclose(host(g.nat1), o.nat1, rtol=1e-9, atol=1e-9 * np.abs(o.nat1).max())
        np.testing.assert_allclose(host(g.nat2), o.nat2, rtol=1e-9, atol=1e-9 * np.abs(o.nat2).max())
        np.testing.assert_allclose(float(g.classic_elbo(data)), o.classic_elbo(t, y), rtol=1e-9)


def test_piecewise_kernel_takes_leg_children(amd, rng):
    """PiecewiseKernel over two Sum([LEG, Matern32]) children with their own parameters (PiecewiseKernel admits children of one class
    only, so the LEG and the Matern sit together in each region's Sum) builds through the region-selected torch route and matches
    tests/np_piecewise.py at the tolerances of test_gpu_piecewise.py::test_torch_route_matches_numpy."""
    from tests import np_piecewise as PW
    from vidp_amd import kernels as K
    NR = [(rng.random((2, 2)) + np.eye(2), rng.random((2, 2))) for _ in range(2)]
    ls = [0.6, 1.4]
    gk = K.PiecewiseKernel([K.Sum([K.LatentExponentiallyGenerated(N, R), K.Matern32(l, 1.2)]) for (N, R), l in zip(NR, ls)], [1.5],
                           jitter=1e-6)
    ok = PW.PiecewiseKernel([np_kernels.Sum([L.LatentExponentiallyGenerated(N, R), np_kernels.Matern32(l, 1.2)])
                             for (N, R), l in zip(NR, ls)], [1.5], jitter=1e-6)
    t = np.sort(np.concatenate([[1.5], rng.uniform(0.0, 3.0, size=(24,))]))[None].repeat(2, axis=0)
    _, oP0, oA, ob, oQ = ok.ssm_parameters(t)
    scale = max(np.abs(k.steady_state_covariance()).max() for k in ok.kernels)
    g = gk.state_space_model(dev(t))
    assert gk.state_dim == 4
    np.testing.assert_allclose(host(g.state_transitions), oA, rtol=0, atol=1e-12 * max(1.0, np.abs(oA).max()))
    np.testing.assert_allclose(host(g.state_offsets), ob, rtol=0, atol=1e-12 * max(1.0, np.abs(ob).max()))
    c = host(g.cholesky_process_covariances)
    np.testing.assert_allclose(c @ np.swapaxes(c, -1, -2), oQ, rtol=0, atol=1e-12 * scale)
    c0 = host(g.cholesky_initial_covariance)
    np.testing.assert_allclose(c0 @ np.swapaxes(c0, -1, -2), oP0, rtol=0, atol=1e-12 * scale)


def test_piecewise_kernel_of_two_legs(amd, rng):
    """PiecewiseKernel([LEG, LEG], [t*]) with different N, R and state means per region: a LEG child directly under the piecewise
    kernel, through the region-selected torch route, against tests/np_piecewise.py at the same tolerances."""
    from tests import np_piecewise as PW
    from vidp_amd import kernels as K
    d = 3
    NR = [(rng.random((d, d)) + np.eye(d), rng.random((d, d))) for _ in range(2)]
    means = [rng.normal(size=d) for _ in range(2)]
    gkids, okids = [], []
    for (N, R), m in zip(NR, means):
        g, o = pair(N, R)
        g.set_state_mean(m)
        o._state_mean = m
        gkids.append(g)
        okids.append(o)
    gk, ok = K.PiecewiseKernel(gkids, [1.5], jitter=1e-6), PW.PiecewiseKernel(okids, [1.5], jitter=1e-6)
    t = np.sort(np.concatenate([[1.5], rng.uniform(0.0, 3.0, size=(24,))]))[None].repeat(2, axis=0)
    _, oP0, oA, ob, oQ = ok.ssm_parameters(t)
    g = gk.state_space_model(dev(t))
    np.testing.assert_allclose(host(g.state_transitions), oA, rtol=0, atol=1e-12 * max(1.0, np.abs(oA).max()))
    np.testing.assert_allclose(host(g.state_offsets), ob, rtol=0, atol=1e-12 * max(1.0, np.abs(ob).max()))
    c = host(g.cholesky_process_covariances)
    np.testing.assert_allclose(c @ np.swapaxes(c, -1, -2), oQ, rtol=0, atol=1e-12)
    c0 = host(g.cholesky_initial_covariance)
    np.testing.assert_allclose(c0 @ np.swapaxes(c0, -1, -2), oP0, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(host(g.initial_mean), np.zeros((2, d)))


def test_hyperparameter_tape_against_finite_differences(amd, rng):
    """CVIGaussianProcess with a Gaussian likelihood after one learning_rate = 1 site update: the optimal sites do not depend on the
    kernel, so classic_elbo is the GPR log marginal likelihood of every (N, R).  Its tape gradients with respect to N and R (d = 2,
    T = 25) against central differences (step 1e-5) of the dense-GP log marginal likelihood built from np_leg's k(tau): relative 1e-6
    of the largest entry of each gradient (the diagonal of dL/dR is exactly zero, R enters through R - R^T)."""
    import torch
    from vidp_amd.likelihoods import Gaussian
    from vidp_amd.variational_cvi import CVIGaussianProcess
    N, R = rng.random((2, 2)) + np.eye(2), rng.random((2, 2))
    t = np.cumsum(rng.uniform(0.1, 0.4, size=25))
    y = np.sin(2 * t)[:, None] + 0.1 * rng.normal(size=(25, 1))
    noise = 0.4
    gk, _ = pair(N, R)
    g = CVIGaussianProcess((dev(t), dev(y)), gk, Gaussian(noise), learning_rate=1.0)
    g.update_sites()
    elbo, leaves = g.classic_elbo_tape_hyper()

    def ref(Nv, Rv):
        ok = L.LatentExponentiallyGenerated(Nv, Rv)
        return _dense_logml(L.dense_k(ok, t[:, None] - t[None, :]), y, noise)
    np.testing.assert_allclose(float(elbo.detach()), ref(N, R), rtol=1e-8)
    gN, gR = torch.autograd.grad(elbo, [leaves["N"], leaves["R"]])
    e = 1e-5
    for which, gr in (("N", host(gN)), ("R", host(gR))):
        fd = np.zeros((2, 2))
        for i in range(2):
            for j in range(2):
                def at(s):
                    M = [N.copy(), R.copy()]
                    M[0 if which == "N" else 1][i, j] += s
                    return ref(*M)
                fd[i, j] = (at(e) - at(-e)) / (2 * e)
        print(f"d/d{which}: tape {gr.tolist()} fd {fd.tolist()}")
        np.testing.assert_allclose(gr, fd, rtol=0, atol=1e-6 * np.abs(fd).max())
