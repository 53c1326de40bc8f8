"""
Host tests of Gaussian-process factor analysis (vidp_amd.kernels.FactorAnalysisKernel, vidp_amd.factor_analysis_variational.
FactorAnalysisSparseCVI) on the torch route with CPU tensors: the emission matrix, a known answer (the conjugate model against the dense
GP log marginal of tests/np_fa.py), the model against the dense NumPy model, the decomposition into scalar sparse CVI models at W = I,
loading_grad against autograd, the rotation invariance of the Gaussian model, constructor refusals, and the argument checks of the
three C entry points (which return before any launch).
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import np_kernels
from tests import np_fa, np_ml

T = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))


def kids2(K):
    return [K.Matern32(1.0, 1.0), K.Matern52(0.8, 0.7)]


def weight_fn_np(t):
    """A(t) [N, 3, 2], smooth in time."""
    t = np.asarray(t)
    return np.stack([np.stack([1.0 + 0.3 * np.sin(0.5 * t), 0.4 * np.cos(0.3 * t)], -1),
                     np.stack([0.5 * np.cos(0.2 * t), 0.9 + 0.0 * t], -1),
                     np.stack([-0.6 + 0.1 * t / (1.0 + np.abs(t)), 0.7 * np.sin(0.4 * t)], -1)], -2)


def weight_fn(t):
    return torch.from_numpy(weight_fn_np(t.detach().cpu().numpy())).to(t.device)


def test_emission_matrix_is_weights_times_block_diagonal_emission():
    """generate_emission_model(t).emission_matrix = A(t) B (H_1 (+) H_2) for constant and callable weights (the reference's
    test_factor_analysis_kernel_emission_model); constant weights carry constant_matrix."""
    from vidp_amd import kernels as K
    rng = np.random.default_rng(0)
    t = np.sort(rng.uniform(0, 10, size=17))
    B = rng.normal(size=(2, 2))
    H = np.zeros((2, 5))
    H[0, 0] = H[1, 2] = 1.0
    A = rng.normal(size=(3, 2))
    for wf, At in ((T(A), np.broadcast_to(A, (17, 3, 2))), (weight_fn, weight_fn_np(t))):
        k = K.FactorAnalysisKernel(wf, kids2(K), 3)
        assert k.state_dim == 5 and k.output_dim == 3 and k.latent_dim == 2
        assert torch.equal(k.loading_matrix, torch.eye(2, dtype=torch.float64))
        np.testing.assert_allclose(k.generate_emission_model(T(t)).emission_matrix.numpy(), At @ H, rtol=1e-15, atol=0)
        k.assign_loading_matrix(T(B))
        em = k.generate_emission_model(T(t))
        assert tuple(em.emission_matrix.shape) == (17, 3, 5)
        np.testing.assert_allclose(em.emission_matrix.numpy(), At @ B @ H, rtol=1e-14, atol=1e-15)
        np.testing.assert_allclose(k.weights(T(t)).numpy(), (At @ B)[0] if k.constant_weights else At @ B, rtol=1e-14, atol=1e-15)
        assert (em.constant_matrix is not None) == k.constant_weights
    assert isinstance(k.latent_components, K.IndependentMultiOutput) and k.latent_components.output_dim == 2
    vals = k.hyperparameter_values()
    vals[0]["lengthscale"] = 2.5
    k.assign_hyperparameters(vals)
    assert k.kernels[0].lengthscale == 2.5 and k.latent_components.kernels[0].lengthscale == 2.5


def test_conjugate_model_recovers_the_dense_log_marginal():
    """Known answer.  Gaussian likelihood, jitter 0, inducing points = the data times, lr = 1: one update_sites from the initial sites
    is exact, so classic_elbo is the log marginal likelihood of the GP -- compared with the dense covariance of tests/np_fa.py (no
    state-space code) at the project's model-versus-restatement rtol 1e-8.  N = 40, L = 2 (Matern32 + Matern52), P = 5, a quarter of
    the entries NaN.  With half as many inducing points the bound is strictly lower."""
    import vidp_amd
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Gaussian
    rng = np.random.default_rng(3)
    N, P, L, s2 = 40, 5, 2, 0.3
    t = 0.3 * np.arange(N) + rng.uniform(0.0, 0.1, size=N)
    A, B = rng.normal(size=(P, L)), np.array([[1.0, 0.4], [-0.3, 0.8]])
    Y = rng.normal(size=(N, P))
    Y[rng.uniform(size=(N, P)) < 0.25] = np.nan
    assert 30 < np.isnan(Y).sum() < 70
    want = np_fa.gp_log_marginal(kids2(np_kernels), t, Y, np_fa.weights(A, B, t), s2)
    data = (T(t), T(Y))
    got = []
    for z in (t, t[::2]):
        k = K.FactorAnalysisKernel(T(A), kids2(K), P)
        k.assign_loading_matrix(T(B))
        m = vidp_amd.FactorAnalysisSparseCVI(k, T(z), Gaussian(s2), learning_rate=1.0)
        m.update_sites(data)
        got.append(float(m.classic_elbo(data)))
    print(f"fa known answer: elbo {got[0]!r} dense log marginal {want!r}; half the inducing points {got[1]!r}")
    np.testing.assert_allclose(got[0], want, rtol=1e-8)
    assert got[1] < got[0] - 1e-6 * abs(want)


def _case(rng, kind):
    """(A for the model, A for the oracle, likelihood, oracle likelihoods, t, Y) of the torch-route test: constant weights with the
    Poisson likelihood, time-varying ones with the Bernoulli likelihood."""
    from vidp_amd.likelihoods import Bernoulli, Poisson
    z = 0.25 * np.arange(40.0)
    t = np.sort(rng.uniform(z[0] - 0.3, z[-1] + 0.3, size=300))
    if kind == "poisson":
        A = 0.6 * rng.normal(size=(3, 2))
        Y = rng.poisson(np.exp(0.4 * np.sin(0.3 * t)[:, None] + 0.1 * np.arange(3)), size=(300, 3)).astype(np.float64)
        lik, oliks, Am, Ao = Poisson(1.3), [np_fa.make_lik(np_fa.POISSON, 1.3)] * 3, T(A), A
    else:
        Y = (rng.uniform(size=(300, 3)) < 0.5 + 0.4 * np.sin(0.5 * t)[:, None]).astype(np.float64)
        lik, oliks, Am, Ao = Bernoulli(1e-3), [np_fa.make_lik(np_fa.BERNOULLI, 1e-3)] * 3, weight_fn, weight_fn_np
    Y[rng.uniform(size=Y.shape) < 0.1] = np.nan
    return z, t, Y, lik, oliks, Am, Ao


@pytest.mark.parametrize("kind", ["poisson", "bernoulli"])
def test_torch_route_against_dense_numpy(kind):
    """40 inducing points 0.25 lengthscales apart, 300 points, P = 3, twenty damped steps (lr = 0.5): sites, ELBO, predict_f and
    predict_latents (diagonal and full) at unsorted new times against tests/np_fa.py at 1e-8."""
    import vidp_amd
    from vidp_amd import kernels as K
    rng = np.random.default_rng(7)
    z, t, Y, lik, oliks, Am, Ao = _case(rng, kind)
    B = np.array([[0.9, -0.2], [0.3, 1.1]])
    k = K.FactorAnalysisKernel(Am, kids2(K), 3)
    k.assign_loading_matrix(T(B))
    m = vidp_amd.FactorAnalysisSparseCVI(k, T(z), lik, learning_rate=0.5)
    o = np_fa.FactorAnalysisSparseCVI(kids2(np_kernels), z, Ao, B, oliks, learning_rate=0.5)
    data = (T(t), T(Y))
    tol = 1e-8
    for step in range(20):
        m.update_sites(data)
        o.update_sites(t, Y)
        np.testing.assert_allclose(m.nat1.numpy(), o.nat1, rtol=tol, atol=tol * np.abs(o.nat1).max())
        np.testing.assert_allclose(m.nat2.numpy(), o.nat2, rtol=tol, atol=tol * np.abs(o.nat2).max())
        em, eo = float(m.elbo(data)), o.elbo(t, Y)
        if step in (0, 19):
            print(f"fa host {kind} step {step}: elbo torch {em!r} numpy {eo!r}")
        np.testing.assert_allclose(em, eo, rtol=tol)
    assert float(m.loss(data)) == -float(m.classic_elbo(data))
    tn = rng.uniform(z[0] - 0.5, z[-1] + 0.5, size=150)          # unsorted new times
    for tt, (fm, fv) in ((t, m.predict_f_at_data(data)), (tn, m.predict_f(T(tn)))):
        om, ov = o.predict_f(tt)
        assert tuple(fm.shape) == (len(tt), 3)
        np.testing.assert_allclose(fm.numpy(), om, rtol=tol, atol=tol)
        np.testing.assert_allclose(fv.numpy(), ov, rtol=tol, atol=tol)
    om, oK = o.predict_latents(tn)
    lm, lv = m.predict_latents(T(tn))
    lm2, lK = m.predict_latents(T(tn), full_cov=True)
    assert tuple(lv.shape) == (150, 2) and tuple(lK.shape) == (150, 2, 2) and torch.equal(lm, lm2)
    np.testing.assert_allclose(lm.numpy(), om, rtol=tol, atol=tol)
    np.testing.assert_allclose(lK.numpy(), oK, rtol=tol, atol=tol)
    np.testing.assert_allclose(lv.numpy(), np.diagonal(oK, axis1=-2, axis2=-1), rtol=tol, atol=tol)
    assert np.abs(oK[:, 0, 1]).max() > 1e-3          # the mixing correlates the latents a posteriori
    lp = m.predict_log_density(data)
    assert tuple(lp.shape) == (300,) and bool(torch.isfinite(lp).all())


def test_identity_weights_decompose_into_scalar_models():
    """P = L and W = I: the model is L scalar sparse CVI models side by side (model l on the times where channel l is observed) --
    site blocks equal, cross-latent site blocks exactly zero, ELBO = the sum of the scalar ELBOs, at 1e-8 over twenty damped steps."""
    import vidp_amd
    from tests.test_host_ml import scalar_model
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Bernoulli, Poisson
    rng = np.random.default_rng(11)
    z = 0.25 * np.arange(40.0)
    t = np.sort(rng.uniform(z[0] - 0.3, z[-1] + 0.3, size=400))
    Y = np.stack([(rng.uniform(size=400) < 0.5 + 0.4 * np.sin(0.5 * t)).astype(np.float64),
                  rng.poisson(np.exp(0.4 * np.cos(0.3 * t))).astype(np.float64)], 1)
    Y[rng.uniform(size=Y.shape) < 0.1] = np.nan
    liks = [Bernoulli(1e-3), Poisson(1.3)]
    m = vidp_amd.FactorAnalysisSparseCVI(K.FactorAnalysisKernel(torch.eye(2, dtype=torch.float64), kids2(K), 2), T(z), liks,
                                         learning_rate=0.5)
    parts, pdata = [], []
    for l, (k, lik) in enumerate(zip(kids2(K), [Bernoulli(1e-3), Poisson(1.3)])):
        sel = ~np.isnan(Y[:, l])
        parts.append(scalar_model(k, z, lik, 0.5))
        pdata.append((T(np.stack([np.zeros(sel.sum()), t[sel]], 1)), T(Y[sel, l][:, None])))
    data = (T(t), T(Y))
    dl = [2, 3]
    D, off = 5, np.array([0, 2, 5])
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
    print(f"fa decomposition: elbo {float(m.elbo(data))!r} sum of the scalar models {total!r}")


def test_loading_grad_against_autograd():
    """loading_grad (the closed form on the latent marginals and the likelihood derivatives) against torch autograd through the
    torch route's sum of variational expectations as a function of B, at 1e-10 of the sum of absolute terms
    sum_ip |A_ipk| (|dm a_l| + 2 |dv| sum_l' |W_pl'| |K_ll'|).  Mixed likelihoods, time-varying weights, NaN entries, sites after three
    damped steps."""
    import vidp_amd
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Bernoulli, Gaussian, Poisson
    rng = np.random.default_rng(13)
    z = 0.25 * np.arange(30.0)
    t = np.sort(rng.uniform(z[0] - 0.3, z[-1] + 0.3, size=200))
    Y = np.stack([rng.normal(size=200), (rng.uniform(size=200) < 0.5).astype(np.float64), rng.poisson(1.0, size=200).astype(np.float64)], 1)
    Y[rng.uniform(size=Y.shape) < 0.1] = np.nan
    k = K.FactorAnalysisKernel(weight_fn, kids2(K), 3)
    B = np.array([[0.9, -0.2], [0.3, 1.1]])
    k.assign_loading_matrix(T(B))
    m = vidp_amd.FactorAnalysisSparseCVI(k, T(z), [Gaussian(0.5), Bernoulli(1e-3), Poisson(0.8)], learning_rate=0.5)
    data = (T(t), T(Y))
    for _ in range(3):
        m.update_sites(data)
    got = m.loading_grad(data).numpy()
    Bt = T(B).requires_grad_(True)
    (want,) = torch.autograd.grad(m.ve_sum_torch(data, Bt), [Bt])
    fmu, fvar, Wn = m._predict_torch(T(t))[:3]
    _, dm, dv = m._lik_terms(fmu, fvar, T(Y))
    lmu, Kf = m._latents_torch(T(t))
    sdW = dm.abs()[:, :, None] * lmu.abs()[:, None, :] + 2.0 * dv.abs()[:, :, None] * torch.einsum("npk,nlk->npl", Wn.abs(), Kf.abs())
    scale = torch.einsum("npk,npl->kl", T(weight_fn_np(t)).abs(), sdW).numpy()
    err = np.max(np.abs(got - want.numpy()) / (1e-10 * scale))
    print(f"fa loading_grad: |closed form - autograd| / (1e-10 sum|terms|) = {err:.3e}; grad {got.tolist()}")
    assert tuple(got.shape) == (2, 2) and np.abs(got).min() > 1e-3
    assert err <= 1.0


def test_rotating_identical_latents_leaves_the_gaussian_elbo_unchanged():
    """With identical children the prior of the latents is invariant under an orthogonal R, so B -> B R describes the same model: the
    exact bound of the Gaussian model (one lr = 1 step each) agrees at 1e-8."""
    import vidp_amd
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Gaussian
    rng = np.random.default_rng(17)
    z = 0.25 * np.arange(30.0)
    t = np.sort(rng.uniform(z[0] - 0.3, z[-1] + 0.3, size=150))
    Y = rng.normal(size=(150, 4))
    Y[rng.uniform(size=Y.shape) < 0.1] = np.nan
    A = rng.normal(size=(4, 3))
    B = rng.normal(size=(3, 3))
    R = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    data = (T(t), T(Y))
    got = []
    for Bk in (B, B @ R):
        k = K.FactorAnalysisKernel(T(A), [K.Matern32(0.9, 1.2) for _ in range(3)], 4)
        k.assign_loading_matrix(T(Bk))
        m = vidp_amd.FactorAnalysisSparseCVI(k, T(z), Gaussian(0.4), learning_rate=1.0)
        m.update_sites(data)
        got.append(float(m.classic_elbo(data)))
    print(f"fa rotation: elbo {got[0]!r} rotated {got[1]!r}")
    np.testing.assert_allclose(got[0], got[1], rtol=1e-8)


def test_constructor_refusals():
    import vidp_amd
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Bernoulli, Gaussian
    cls = vidp_amd.FactorAnalysisSparseCVI
    z = T(np.arange(5.0))
    A = torch.ones((3, 2), dtype=torch.float64)
    k = K.FactorAnalysisKernel(A, kids2(K), 3)
    with pytest.raises(NotImplementedError, match="mean_function"):
        cls(k, z, Gaussian(1.0), mean_function=lambda t: t)
    with pytest.raises(NotImplementedError, match="shard"):
        cls(k, z, Gaussian(1.0), shard=(0, 2))
    with pytest.raises(TypeError, match="FactorAnalysisKernel"):
        cls(K.IndependentMultiOutput(kids2(K)), z, Gaussian(1.0))
    with pytest.raises(ValueError, match="must agree"):
        cls(k, z, [Gaussian(1.0), Bernoulli()])
    with pytest.raises(NotImplementedError, match="batched"):
        cls(k, z[None].repeat(2, 1), Gaussian(1.0))
    wide = K.FactorAnalysisKernel(A, [K.Sum([K.Matern52(1.0, 1.0)] * 6), K.Sum([K.Matern52(1.0, 1.0)] * 5)], 3)
    with pytest.raises(ValueError, match="state dimension 33"):
        cls(wide, z, Gaussian(1.0))
    with pytest.raises(ValueError, match="state dimension 1 "):
        cls(K.FactorAnalysisKernel(torch.ones((3, 1), dtype=torch.float64), [K.Matern12(1.0, 1.0)], 3), z, Gaussian(1.0))
    pw = K.PiecewiseKernel([K.Matern32(1.0, 1.0), K.Matern32(2.0, 1.0)], T(np.array([2.0])))
    with pytest.raises(NotImplementedError, match="PiecewiseKernel"):
        K.FactorAnalysisKernel(A, [pw, K.Matern32(1.0, 1.0)], 3)
    leg = K.LatentExponentiallyGenerated(np.eye(2), np.zeros((2, 2)))
    with pytest.raises(NotImplementedError, match="LEG"):
        K.FactorAnalysisKernel(A, [leg, K.Matern32(1.0, 1.0)], 3)
    with pytest.raises(ValueError, match="constant weights"):
        K.FactorAnalysisKernel(torch.ones((2, 3), dtype=torch.float64), kids2(K), 3)
    with pytest.raises(ValueError, match="loading matrix"):
        k.assign_loading_matrix(torch.eye(3, dtype=torch.float64))
    bad = K.FactorAnalysisKernel(lambda t: torch.ones(tuple(t.shape) + (2, 2), dtype=torch.float64), kids2(K), 3)
    with pytest.raises(ValueError, match="weight_function must return"):
        bad.weights(z)
    m = cls(k, z, Gaussian(1.0))
    assert m.latent_dim == 2 and m.output_dim == 3 and m.kernel is k and m.nat1.shape == (6, 10) and m.nat2.shape == (6, 10, 10)
    with pytest.raises(NotImplementedError, match="elbo_and_grad"):
        m.elbo_and_grad((z, torch.zeros((5, 3), dtype=torch.float64)))
    with pytest.raises(NotImplementedError, match="device"):
        m.dist_q
    with pytest.raises(NotImplementedError, match="device route"):
        m.step_graph((z, torch.zeros((5, 3), dtype=torch.float64)))


def test_entry_points_check_their_arguments_without_a_gpu():
    """mfgm_fa_predict_lik / mfgm_fa_site_update / mfgm_fa_site_update_q return 1 before any launch for L outside 1 .. 8, P outside
    1 .. 64, a dl < 1, D outside 2 .. 32, a w_stride other than 0 or P L, an unknown kind, kinds that are 0 for some outputs only, a
    parameter out of range, lr outside [0, 1] and a missing pointer when N > 0; N = 0 prediction returns 0."""
    import vidp_amd
    lib = vidp_amd._lib.load()
    one = ctypes.c_void_p(8)          # a non-null pointer that is never dereferenced: every call below fails its checks first

    def fa(dl, P=3, M=4, N=3, L=None, stride=0, seg=one, h=one, c=one, w=one, pm=one, pc=one):
        s = vidp_amd._lib.FaData()
        s.M, s.L, s.P, s.N = M, len(dl) if L is None else L, P, N
        for k, n in enumerate(dl[:8]):
            s.dl[k] = n
        s.seg, s.h, s.c, s.w, s.w_stride, s.prior_mean, s.prior_cov = seg, h, c, w, stride, pm, pc
        return s

    def lk(kinds, params=None, P=3):
        q = vidp_amd._lib.FaLik()
        for p in range(P):
            q.kind[p] = kinds if isinstance(kinds, int) else kinds[p]
            q.param[p] = {0: 0.0, 1: 1e-3, 2: 1.0, 3: 0.5}.get(q.kind[p], 1.0) if params is None else params
        return q

    def predict(s, q=None, y=None, mu=one, ve=None, dm=None, dv=None, g1=None, g2=None):
        q = lk(0) if q is None else q
        return lib.mfgm_fa_predict_lik(ctypes.byref(s), ctypes.byref(q), y, mu, one, one, one, one, one, one, ve, dm, dv, g1, g2, None)

    def update(s, lr=0.5, g1=one, g2=one, nat1=one, nat2=one, packed=False):
        fn = lib.mfgm_fa_site_update_q if packed else lib.mfgm_fa_site_update
        return fn(ctypes.byref(s), g1, g2, lr, nat1, nat2, None)

    bad_shapes = [dict(dl=[1]), dict(dl=[16, 17]), dict(dl=[2, 0]), dict(dl=[2, -1, 4]), dict(dl=[4] * 8, L=9), dict(dl=[2, 2], L=0),
                  dict(dl=[2 ** 30, 2 ** 30, 2 ** 30, 2 ** 30]), dict(dl=[33]), dict(dl=[2, 2], M=0), dict(dl=[2, 2], N=-1),
                  dict(dl=[2, 2], P=0), dict(dl=[2, 2], P=65), dict(dl=[2, 2], P=-1), dict(dl=[2, 2], stride=5), dict(dl=[2, 2], stride=3),
                  dict(dl=[2, 2], stride=-6), dict(dl=[2, 2], seg=None), dict(dl=[2, 2], h=None), dict(dl=[2, 2], c=None)]
    for kw in bad_shapes:
        s = fa(**kw)
        assert predict(s) == 1 and update(s) == 1 and update(s, packed=True) == 1, kw
    ok = fa([2, 1, 3])
    assert fa([2, 2], stride=6).w_stride == 6
    for q in (lk(4), lk(-1), lk([1, 0, 2]), lk([0, 0, 3])):                      # unknown kinds; kinds that are 0 for some outputs only
        assert predict(ok, q, y=one, ve=one) == 1
    for kind, prm in ((1, -1e-3), (1, 0.5), (1, float("nan")), (2, 0.0), (2, -1.0), (2, float("nan")), (2, float("inf")), (3, 0.0),
                      (3, -0.5), (3, float("inf")), (3, float("nan"))):
        assert predict(ok, lk(kind, prm), y=one, ve=one) == 1, (kind, prm)
    assert predict(ok, lk([1, 2, 3]), y=None, ve=one) == 1                     # a likelihood needs y
    for out in ("ve", "dm", "dv", "g1", "g2"):                                   # no likelihood: no likelihood outputs
        assert predict(ok, lk(0), **{out: one}) == 1
    assert predict(ok, lk(0), y=one) == 1
    assert predict(ok, mu=None) == 1 and predict(fa([2, 1, 3], pm=None)) == 1 and predict(fa([2, 1, 3], pc=None)) == 1
    assert predict(fa([2, 1, 3], w=None)) == 1
    for lr in (-0.1, 1.5, float("nan")):
        assert update(ok, lr=lr) == 1 and update(ok, lr=lr, packed=True) == 1
    for packed in (False, True):
        for miss in ("g1", "g2", "nat1", "nat2"):
            assert update(ok, packed=packed, **{miss: None}) == 1
    q0 = lk(0)
    assert lib.mfgm_fa_predict_lik(None, ctypes.byref(q0), None, one, one, one, one, one, one, one, None, None, None, None, None, None) == 1
    assert lib.mfgm_fa_predict_lik(ctypes.byref(ok), None, None, one, one, one, one, one, one, one, None, None, None, None, None, None) == 1
    assert lib.mfgm_fa_site_update(None, one, one, 0.5, one, one, None) == 1
    # no data: prediction has nothing to do, with or without a likelihood
    empty = fa([2, 1, 3], N=0, h=None, c=None, w=None)
    assert predict(empty) == 0 and predict(empty, lk([1, 2, 3]), ve=one) == 0
