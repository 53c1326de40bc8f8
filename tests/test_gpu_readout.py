"""
GPU tests of the linear-readout likelihood of the diffusion models (vidp_amd.likelihoods.LinearReadout; kernels
mfgm_readout_site_update / mfgm_readout_obs_ve, csrc/mfgm_readout.h): the two entry points through Plan against the NumPy restatement
tests/np_readout.py, CVISitesSSM / CVISitesSDE with a readout against the restated oracle models, the native route against the torch
route, two known answers (the GP model with the same kernel; MultivariateGaussian at H = I) and the trainer's metrics.  fp64.
"""
import numpy as np
import pytest

from oracle import np_kernels, np_sde
from tests import np_lik, np_readout

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


def within(got, want, scale, what):
    err = np.abs(np.asarray(got) - want)
    print(f"{what}: worst error / scale = {np.max(err / np.maximum(scale, 1e-300)):.3g}")
    assert np.all(err <= 1e-12 * scale), what


# ---- the two entry points ------------------------------------------------------------------------------------------------------------
B_K, T_K, N_PER = 3, 320, 300      # R0 = 4: 240 level-0 lanes (node blocks beyond the first 64-lane tile); 300 > 256: two partial sums


def _nodes(rng):
    """[B, n_per] distinct unsorted nodes per chain, among them 0, T - 1 and both ends of a segment (3 | 4)."""
    keep = np.array([0, 3, 4, T_K - 1])
    rest = np.setdiff1d(np.arange(T_K), keep)
    return np.stack([rng.permutation(np.concatenate([keep, rng.permutation(rest)[:N_PER - len(keep)]])) for _ in range(B_K)])


@pytest.mark.parametrize("which_o", ["one", "two", "d+1"])
@pytest.mark.parametrize("d", [1, 2, 3, 6, 8])
def test_entry_points_match_numpy(amd, rng, d, which_o):
    """mfgm_readout_site_update (lr 1.0 and 0.3, marginals from the packed arrays and gathered) and mfgm_readout_obs_ve (with and without
    the gathered outputs) against the restatement: sites and the posterior naturals at the listed nodes within 1e-12 of the sum of the
    absolute terms they are made of, everything else in the packed arrays (other nodes, padding lanes) bit-identical, the
    per-trajectory sums to rtol 1e-12."""
    import torch
    o = {"one": 1, "two": 2, "d+1": min(d + 1, 8)}[which_o]
    kinds = ("gpb" * 2)[d % 3:d % 3 + 3]
    H, c, spec, ref = np_readout.random_readout(rng, d, o, kinds)
    from vidp_amd import likelihoods as L
    rd = np_readout.torch_readout(L, H, c, spec).descriptor()
    plan = amd.Plan(B_K, T_K, d, R0=4)
    assert plan.Lpad >= 240 and plan.R == 4
    t_idx = _nodes(rng)
    flat = (np.arange(B_K)[:, None] * T_K + t_idx).reshape(-1)
    ids = torch.from_numpy(flat).cuda()
    n = flat.size
    mu, cov = np_readout.random_marginals(rng, B_K * T_K, d)
    y = np_readout.random_observations(rng, ref, mu[flat])
    y[5] = np.nan
    (ve, g1, g2), (sv, s1, s2) = ref.all_with_scales(mu[flat], cov[flat], y)
    assert ve[5] == 0.0
    pm, pc = plan.pack(amd.VEC, dev(mu.reshape(B_K, T_K, d))), plan.pack(amd.SYM, dev(cov.reshape(B_K, T_K, d, d)))
    # which packed entries belong to a listed node (padding lanes and the other nodes: 0)
    sel = np.zeros(B_K * T_K)
    sel[flat] = 1.0
    mask_v = plan.pack(amd.VEC, dev(np.repeat(sel[:, None], d, 1).reshape(B_K, T_K, d))) != 0
    mask_s = plan.pack(amd.SYM, dev(np.repeat(sel[:, None], d * d, 1).reshape(B_K, T_K, d, d))) != 0
    th1 = rng.normal(size=(B_K * T_K, d))
    th2 = rng.normal(size=(B_K * T_K, d, d))
    th2 = th2 + np.swapaxes(th2, -1, -2)
    A = rng.normal(size=(n, d, d))
    old1, old2 = rng.normal(size=(n, d)), A + np.swapaxes(A, -1, -2)
    yd = dev(y)
    for lr in (1.0, 0.3):
        for gathered in (False, True):
            # padding lanes carry a sentinel of their own
            p1 = torch.full_like(pm, 7.0)
            p2 = torch.full_like(pc, 7.0)
            p1 = torch.where(plan.pack(amd.VEC, torch.ones((B_K, T_K, d), dtype=torch.float64, device="cuda")) != 0,
                             plan.pack(amd.VEC, dev(th1.reshape(B_K, T_K, d))), p1)
            p2 = torch.where(plan.pack(amd.SYM, torch.ones((B_K, T_K, d, d), dtype=torch.float64, device="cuda")) != 0,
                             plan.pack(amd.SYM, dev(th2.reshape(B_K, T_K, d, d))), p2)
            b1, b2 = p1.clone(), p2.clone()
            s1d, s2d = dev(old1), dev(old2)
            if gathered:
                plan.readout_site_update(rd, dev(mu[flat]), dev(cov[flat]), ids, yd, p1, p2, s1d, s2d, lr, gathered=True)
            else:
                plan.readout_site_update(rd, pm, pc, ids, yd, p1, p2, s1d, s2d, lr)
            torch.cuda.synchronize()
            new1, new2 = (1 - lr) * old1 + lr * g1, (1 - lr) * old2 + lr * g2
            tag = f"d={d} o={o} lr={lr} gathered={gathered}"
            within(host(s1d), new1, (1 - lr) * np.abs(old1) + lr * s1, "sites_vec " + tag)
            within(host(s2d), new2, (1 - lr) * np.abs(old2) + lr * s2, "sites_sym " + tag)
            np.testing.assert_array_equal(host(s2d), np.swapaxes(host(s2d), -1, -2))
            u1 = host(plan.unpack(amd.VEC, p1)).reshape(-1, d)[flat]
            u2 = host(plan.unpack(amd.SYM, p2)).reshape(-1, d, d)[flat]
            within(u1, th1[flat] + new1 - old1, np.abs(th1[flat]) + (2 - lr) * np.abs(old1) + lr * s1, "theta_lin " + tag)
            within(u2, th2[flat] + new2 - old2, np.abs(th2[flat]) + (2 - lr) * np.abs(old2) + lr * s2, "theta_diag " + tag)
            assert torch.equal(p1[~mask_v], b1[~mask_v]) and torch.equal(p2[~mask_s], b2[~mask_s])
            # the all-NaN row: the gradient is exactly zero, so lr = 1 leaves exactly zero sites
            if lr == 1.0:
                assert not host(s1d)[5].any() and not host(s2d)[5].any()
    want = ve.reshape(B_K, N_PER).sum(-1)
    got = plan.readout_obs_ve(rd, pm, pc, ids, N_PER, yd)
    assert got.shape == (B_K,)
    np.testing.assert_allclose(host(got), want, rtol=1e-12)
    om, oc = torch.full((n, d), 7.0, dtype=torch.float64, device="cuda"), torch.full((n, d, d), 7.0, dtype=torch.float64, device="cuda")
    part = plan.readout_obs_ve(rd, pm, pc, ids, N_PER, yd, out_mu=om, out_cov=oc, partials=True)
    assert part.shape == (B_K, 2)
    np.testing.assert_array_equal(host(part.sum(-1)), host(got))
    np.testing.assert_allclose(host(part[:, 0]), ve.reshape(B_K, N_PER)[:, :256].sum(-1), rtol=1e-12)
    np.testing.assert_array_equal(host(om), mu[flat])
    np.testing.assert_array_equal(host(oc), cov[flat])
    within(host(part).sum(), ve.sum(), sv.sum(), f"VE d={d} o={o}")


def test_identity_readout_is_the_multivariate_gaussian_on_the_device(amd, rng):
    """tests/test_host_readout.py's identity with the constructed MultivariateGaussian(s I): VE and both gradients at rtol 1e-12."""
    from vidp_amd import likelihoods as L
    d, s, n = 3, 0.6, 40
    lik, mvn = L.LinearReadout(np.eye(d), L.Gaussian(s * s)), L.MultivariateGaussian(dev(s * np.eye(d)))
    mu, cov = np_readout.random_marginals(rng, n, d)
    y = rng.normal(size=(n, d))
    np.testing.assert_allclose(host(lik.variational_expectations(dev(mu), dev(cov), dev(y))),
                               host(mvn.variational_expectations(dev(mu), dev(cov), dev(y))), rtol=1e-12)
    for a, b in zip(lik.ve_gradients_expectation(dev(mu), dev(cov), dev(y)), mvn.ve_gradients_expectation(dev(mu), dev(cov), dev(y))):
        np.testing.assert_allclose(host(a), host(b), rtol=1e-12, atol=1e-15)


# ---- models --------------------------------------------------------------------------------------------------------------------------
def test_cvi_sites_ssm_against_restatement(amd, rng):
    """CVISitesSSM, Matern-3/2 prior (d = 2), T = 64, B = 2, o = 2 (Poisson + Gaussian): three rounds of update_data_sites(0.5);
    update_girsanov_sites(0.5); classic_elbo() against the restated oracle model per chain (sites and ELBO, rtol 1e-9, the bound of the
    GP models' comparison in tests/test_gpu_lik.py), and the native route against VIDP_NATIVE_READOUT=0 (rtol 1e-11)."""
    import torch
    from vidp_amd import kernels as K, likelihoods as L
    from vidp_amd.variational_cvi_sde import CVISitesSSM
    B, T, d = 2, 64, 2
    t = np.linspace(0.0, 3.0, T)
    idx = np.sort(rng.choice(T, size=11, replace=False))
    H = np.array([[1.0, 0.0], [0.4, -0.3]])
    c = np.array([0.2, -0.1])
    y = np.stack([rng.poisson(2.0, size=(B, len(idx))), rng.normal(size=(B, len(idx)))], -1).astype(np.float64)
    y[0, 2, 1] = np.nan
    mk_lik = lambda: L.LinearReadout(H, [L.Poisson(0.8), L.Gaussian(0.3)], offset=c)
    ref = np_readout.LinearReadout(H, [np_lik.Poisson(0.8), np_readout.Gaussian(0.3)], c)

    def mk(native):
        prior = K.Matern32(0.7, 1.3).state_space_model(dev(np.broadcast_to(t, (B, T))))
        g = CVISitesSSM(prior, t, (t[idx], dev(y)), mk_lik())
        g.native_readout = native
        assert (g.state_dim, g.obs_dim) == (2, 2) and (g._readout_native() is not None) == native
        return g

    a, b = mk(True), mk(False)
    os_ = [np_readout.CVISitesSSM(np_kernels.Matern32(0.7, 1.3).state_space_model(t), t, idx, y[k], ref) for k in range(B)]
    for it in range(3):
        for m in [a, b] + os_:
            m.update_data_sites(0.5)
            m.update_girsanov_sites(0.5)
        ea, eb = host(a.classic_elbo_per_trajectory()), host(b.classic_elbo_per_trajectory())
        eo = np.array([o.classic_elbo() for o in os_])
        print("elbo native", ea, "torch", eb, "oracle", eo)
        np.testing.assert_allclose(ea, eo, rtol=1e-9)
        np.testing.assert_allclose(ea, eb, rtol=1e-11)
        o1, o2 = np.concatenate([o.d1 for o in os_]), np.concatenate([o.d2 for o in os_])
        np.testing.assert_allclose(host(a.data_nat1), o1, rtol=1e-9, atol=1e-9 * np.abs(o1).max())
        np.testing.assert_allclose(host(a.data_nat2), o2, rtol=1e-9, atol=1e-9 * np.abs(o2).max())
        np.testing.assert_allclose(host(a.data_nat1), host(b.data_nat1), rtol=1e-11, atol=1e-11 * np.abs(o1).max())
        np.testing.assert_allclose(host(a.data_nat2), host(b.data_nat2), rtol=1e-11, atol=1e-11 * np.abs(o2).max())
    np.testing.assert_allclose(float(a.classic_elbo()), eo.sum(), rtol=1e-9)
    assert torch.is_tensor(a.variational_expectation()) and a.variational_expectation().shape == (B,)


@pytest.mark.parametrize("which", ["poisson", "bernoulli"])
def test_readout_on_the_kernel_emission_is_the_gp_model(amd, rng, which):
    """Known answer across models: CVISitesSSM on kernel.state_space_model(t) with H = the kernel's emission row and the initial
    posterior path = the prior marginals makes the iteration of CVIGaussianProcess with the same kernel and likelihood; after
    8 x update_data_sites(0.5) / 8 x update_sites() (learning_rate 0.5) the classic ELBOs agree to 1e-7 relative.  The two models start
    their sites at +1e-10 and -1e-10, which cannot be aligned: the NumPy restatements of both (np_readout.CVISitesSSM,
    oracle CVIGaussianProcess; T = 48, Matern-3/2(0.7, 1.3), this test's data) differ by 1.5e-11 (Poisson) and 3.3e-11 (Bernoulli)
    relative, and by up to 9e-10 / 1.7e-9 on other draws of the data; the bound is about 50 times the larger figures."""
    from vidp_amd import kernels as K, likelihoods as L
    from vidp_amd.variational_cvi import CVIGaussianProcess
    from vidp_amd.variational_cvi_sde import CVISitesSSM
    T = 48
    t = np.linspace(0.0, 4.0, T)
    f = 1.5 * np.sin(3 * t)
    if which == "poisson":
        y, mk = rng.poisson(np.exp(f)).astype(np.float64)[:, None], lambda: L.Poisson(1.3)
    else:
        y, mk = (f + 0.5 * rng.normal(size=T) > 0).astype(np.float64)[:, None], lambda: L.Bernoulli()
    kern = K.Matern32(0.7, 1.3)
    prior = kern.state_space_model(dev(t))
    Hrow = host(kern._emission_row())[None]
    m = CVISitesSSM(prior, t, (t, dev(y[None])), L.LinearReadout(Hrow, mk()), initial_posterior_path=prior.marginals)
    assert m._readout_native() is not None
    g = CVIGaussianProcess((dev(t), dev(y)), K.Matern32(0.7, 1.3), mk(), learning_rate=0.5)
    for _ in range(8):
        m.update_data_sites(0.5)
        g.update_sites()
    ea, eb = float(m.classic_elbo()), float(g.classic_elbo())
    print(which, ea, eb, abs(ea - eb) / abs(eb))
    np.testing.assert_allclose(ea, eb, rtol=1e-7)


def _double_well(amd, d, T, B, lik, y, idx, dt=0.02, **kw):
    import torch
    from vidp_amd import sde as gsde
    from vidp_amd.variational_cvi_sde import CVISitesSDE
    grid = np.arange(T) * dt
    init = (np.zeros(d), 0.5 * np.eye(d))
    return CVISitesSDE(gsde.DoubleWellSDE(torch.eye(d, dtype=torch.float64)), grid, (grid[idx], dev(y)), lik, prior_initial_state=init,
                       plan=amd.Plan(B, T, d, R0=8, Rup=3), **kw), grid, init


def test_identity_gaussian_readout_on_cvi_dp_equals_multivariate_gaussian(amd, rng):
    """H = I with Gaussian factors of variance s^2 on CVISitesSDE (double well, d = 2, T = 200, B = 2) against the same model with
    MultivariateGaussian(s I) on the dense arrays (cq_enabled False): ELBO and data sites of two full rounds, rtol 1e-9."""
    from vidp_amd import likelihoods as L
    d, T, B, s = 2, 200, 2, 0.3
    idx = np.arange(5, T - 1, 9)
    y = np.sign(rng.normal(size=(B, len(idx), d))) + 0.2 * rng.normal(size=(B, len(idx), d))
    a, _, _ = _double_well(amd, d, T, B, L.LinearReadout(np.eye(d), L.Gaussian(s * s)), y, idx)
    b, _, _ = _double_well(amd, d, T, B, L.MultivariateGaussian(dev(s * np.eye(d))), y, idx)
    b.cq_enabled = False
    assert a._readout_native() is not None and not a._cq_eligible()
    for lr_d, lr_g in ((0.5, 0.2), (0.3, 0.1)):
        for m in (a, b):
            m.update_data_sites(lr_d)
            m.update_girsanov_sites(lr_g)
        assert a._cq is None and b._cq is None
        np.testing.assert_allclose(host(a.classic_elbo_per_trajectory()), host(b.classic_elbo_per_trajectory()), rtol=1e-9)
        n1, n2 = host(b.data_nat1), host(b.data_nat2)
        np.testing.assert_allclose(host(a.data_nat1), n1, rtol=1e-9, atol=1e-9 * np.abs(n1).max())
        np.testing.assert_allclose(host(a.data_nat2), n2, rtol=1e-9, atol=1e-9 * np.abs(n2).max())


def test_partially_observed_cvi_dp_against_restatement(amd, rng):
    """CVISitesSDE, double well, d = 3 seen through o = 2 outputs (a Gaussian row mixing two coordinates, a Poisson row on the third):
    two rounds of update_data_sites; update_girsanov_sites; classic_elbo against the restated oracle model, with the tolerances of
    tests/test_gpu_api.py::test_cvi_sites_sde (ELBO rtol 1e-6 + atol 1e-6, marginals helpers.assert_close)."""
    from tests.helpers import assert_close
    from vidp_amd import likelihoods as L
    d, T, B = 3, 70, 2
    idx = np.sort(rng.choice(np.arange(1, T), size=8, replace=False))
    H = np.array([[0.8, -0.5, 0.0], [0.0, 0.0, 0.6]])
    c = np.array([0.1, 0.3])
    y = np.stack([rng.normal(size=(B, len(idx))), rng.poisson(2.0, size=(B, len(idx)))], -1).astype(np.float64)
    y[1, 3, 0] = np.nan
    g, grid, init = _double_well(amd, d, T, B, L.LinearReadout(H, [L.Gaussian(0.2), L.Poisson(0.9)], offset=c), y, idx)
    assert (g.state_dim, g.obs_dim) == (3, 2) and g._readout_native() is not None
    ref = np_readout.LinearReadout(H, [np_readout.Gaussian(0.2), np_lik.Poisson(0.9)], c)
    os_ = [np_readout.CVISitesSDE(np_sde.DoubleWellSDE(np.eye(d)), grid, idx, y[b], ref, *init, closed_form=True) for b in range(B)]
    for lr_d, lr_g in ((0.5, 0.2), (0.3, 0.1)):
        g.update_data_sites(lr_d)
        g.update_girsanov_sites(lr_g)
        e = host(g.classic_elbo_per_trajectory())
        for b, o in enumerate(os_):
            o.update_data_sites(lr_d)
            o.update_girsanov_sites(lr_g)
            np.testing.assert_allclose(e[b], o.classic_elbo(), rtol=1e-6, atol=1e-6)
    mu, cov = host(g.fx_mus), host(g.fx_covs)
    for b, o in enumerate(os_):
        assert_close(mu[b], o.fx_mus)
        assert_close(cov[b], o.fx_covs)
        assert_close(host(g.data_nat1).reshape(B, len(idx), d)[b], o.d1)
        assert_close(host(g.data_nat2).reshape(B, len(idx), d, d)[b], o.d2)


def test_trainer_metrics_with_a_readout(amd, rng):
    """CVISitesTrainer with test data under a LinearReadout: NLPD = -mean predict_log_density and RMSE of the predicted output means over
    the observed entries, against the restatement on the oracle model's marginals (rtol 1e-9 on the metrics given the marginals: the
    restatement is evaluated on the device model's own marginals, which the previous test holds to the oracle)."""
    from vidp_amd import likelihoods as L
    from vidp_amd.trainers import CVISitesTrainer
    d, T, B = 2, 90, 2
    idx = np.arange(4, T - 1, 7)
    tidx = np.array([i for i in range(2, T - 1, 5) if i not in set(idx)])
    H, c = np.array([[0.7, 0.4], [0.0, 0.5]]), np.array([0.0, 0.2])
    mk_y = lambda n: np.stack([rng.normal(size=(B, n)), rng.poisson(2.0, size=(B, n))], -1).astype(np.float64)
    y, yt = mk_y(len(idx)), mk_y(len(tidx))
    yt[0, 1, 0] = np.nan
    g, grid, _ = _double_well(amd, d, T, B, L.LinearReadout(H, [L.Gaussian(0.2), L.Poisson(0.9)], offset=c), y, idx)
    ref = np_readout.LinearReadout(H, [np_readout.Gaussian(0.2), np_lik.Poisson(0.9)], c)
    tr = CVISitesTrainer(g, test_data=(grid[tidx], dev(yt)), data_sites_lr=0.5, girsanov_sites_lr=0.2)
    g.update_data_sites(0.5)
    g.update_girsanov_sites(0.2)
    _, nl, rm = tr._elbo_nlpd_rmse()
    mu, cov = host(g.fx_mus)[:, tidx].reshape(-1, d), host(g.fx_covs)[:, tidx].reshape(-1, d, d)
    want_nl, want_rm = np_readout.nlpd_rmse(ref, mu, cov, yt.reshape(-1, 2))
    np.testing.assert_allclose(nl, want_nl, rtol=1e-9)
    np.testing.assert_allclose(rm, want_rm, rtol=1e-9)
    dsum = host(tr._device_sums())
    np.testing.assert_allclose(-dsum[1] / dsum[3], want_nl, rtol=1e-9)
    np.testing.assert_allclose(np.sqrt(dsum[2] / dsum[4]), want_rm, rtol=1e-9)


def test_van_der_pol_seen_through_its_position(amd):
    """CVISitesSDEQuadrature inherits the readout through the dense route: a Van der Pol oscillator (d = 2) observed through its first
    coordinate only (o = 1, Gaussian), two rounds on the native route against the torch route of the same model.  Both routes evaluate
    the same formulas, so they differ by rounding carried through the posterior refresh: rtol 1e-9, the bound this file uses for
    model-level comparisons.  The unobserved coordinate keeps a wider posterior than the observed one."""
    import torch
    from vidp_amd import likelihoods as L, sde as gsde
    from vidp_amd.variational_cvi_sde import CVISitesSDEQuadrature
    r = np.random.default_rng(5)
    T, dt, a0, tau0, qv = 80, 0.01, 1.0, 2.0, 0.05
    x = np.zeros((T, 2))
    x[0] = (1.0, 0.5)
    for t in range(T - 1):
        f = tau0 * np.array([a0 * (x[t, 0] - x[t, 0] ** 3 / 3.0 - x[t, 1]), x[t, 0] / a0])
        x[t + 1] = x[t] + dt * f + np.sqrt(dt * qv) * r.normal(size=2)
    grid = np.arange(T) * dt
    idx = np.arange(2, T - 1, 4)
    y = (x[idx, :1] + 0.02 * r.normal(size=(len(idx), 1)))[None]
    init = (x[0].copy(), 0.05 * np.eye(2))

    def mk(native):
        m = CVISitesSDEQuadrature(gsde.VanderPolOscillatorSDE(1.0, 2.0, torch.from_numpy(qv * np.eye(2))), grid, (grid[idx], dev(y)),
                                  L.LinearReadout(np.array([[1.0, 0.0]]), L.Gaussian(0.02 ** 2)), prior_initial_state=init)
        m.native_readout = native
        assert (m.state_dim, m.obs_dim) == (2, 1) and (m._readout_native() is not None) == native
        return m

    a, b = mk(True), mk(False)
    for lr_d, lr_g in ((0.5, 0.2), (0.3, 0.1)):
        for m in (a, b):
            m.update_data_sites(lr_d)
            m.update_girsanov_sites(lr_g)
        ea, eb = float(a.classic_elbo()), float(b.classic_elbo())
        assert np.isfinite(ea)
        np.testing.assert_allclose(ea, eb, rtol=1e-9)
        n1 = host(b.data_nat1)
        np.testing.assert_allclose(host(a.data_nat1), n1, rtol=1e-9, atol=1e-9 * np.abs(n1).max())
    a.plan.check_info()
    # the sites act on the observed coordinate alone: rows and columns of the other one carry only the initial 1e-10 I
    n2 = host(a.data_nat2)
    assert np.abs(n2[:, 0, 0]).min() > 1.0 and np.abs(n2[:, 1, 1]).max() < 1e-9 and np.abs(n2[:, 0, 1]).max() == 0.0
    cov = host(a.fx_covs)[0, idx]
    assert np.all(cov[:, 1, 1] > cov[:, 0, 0])


def test_repeated_observation_times_raise(amd):
    from vidp_amd import likelihoods as L
    lik = L.LinearReadout(np.ones((1, 2)), L.Poisson())
    with pytest.raises(ValueError, match="repeat"):
        _double_well(amd, 2, 40, 1, lik, np.zeros((1, 3, 1)), np.array([4, 9, 9]))
