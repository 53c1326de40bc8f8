"""
GPU tests of the piecewise-stationary kernel (vidp_amd.kernels.PiecewiseKernel; kernel k_piecewise_ssm, csrc/mfgm_piecewise_ssm.h, entry
point mfgm_packed_piecewise_ssm) against the NumPy restatement tests/np_piecewise.py: the packed SSM for d = 1 .. 8 with change points
inside segments, on time points, before a chain's first point, two between one pair of points and a zero gap on a tie; one region
against mfgm_packed_kernel_ssm; the reference's stitched case; the not-positive-definite report; GPR, prediction across change points,
CVI (Bernoulli), sparse CVI (Poisson), Power EP and the per-region hyper-parameter gradients.  fp64.
"""
import numpy as np
import pytest

from oracle import np_kernels, np_models
from tests import np_kernels_ext as E
from tests import np_lik
from tests import np_piecewise as PW

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


# per-region factors on the lengthscales / periods and on the variances: every region has its own rate and var
LS, VS = [1.0, 0.6, 1.7, 0.8], [1.0, 2.0, 0.5, 1.4]


def child(name, m, x, i):
    """Region i's child of the named case, from the Matern module m and the seasonal module x (vidp_amd.kernels twice, or np_kernels
    and np_kernels_ext)."""
    l, v = LS[i], VS[i]
    P, S, HO = x.Product, m.Sum, x.HarmonicOscillator
    return {
        "m12": lambda: m.Matern12(0.8 * l, 2.0 * v),
        "ho": lambda: HO(1.3 * v, 0.8 * l),
        "m52": lambda: m.Matern52(0.9 * l, 1.1 * v),
        "m32ho": lambda: P([m.Matern32(0.7 * l, 1.3 * v), HO(1.0, 1.5 * l)]),
        "m52_m12ho": lambda: S([m.Matern52(0.5 * l, 1.0 * v), P([m.Matern12(0.8 * l, 2.0 * v), HO(0.7 * v, 0.6 * l)])]),
        "hom32ho": lambda: P([HO(1.0 * v, 3.0 * l), m.Matern32(1.5 * l, 0.8 * v), HO(0.5, 0.7 * l)]),
        "d12": lambda: S([P([m.Matern52(1.2 * l, 0.9 * v), HO(1.0, 2.5 * l)]), P([m.Matern52(0.4 * l, 0.3 * v), HO(0.5 * v, 0.9 * l)])]),
        "m12_ho": lambda: S([m.Matern12(1.0 * l, 1.0 * v), HO(1.0 * v, 1.0 * l)]),
    }[name]()


def set_means(gk, ok, rng):
    """The same random state mean on both kernels (on the children of a Sum, whose mean is theirs)."""
    if type(gk).__name__ == "Sum":
        for g, o in zip(gk.kernels, ok.kernels):
            set_means(g, o, rng)
        return
    m = rng.normal(size=gk.state_dim)
    gk.set_state_mean(m)
    ok._state_mean = m


def piecewise(name, cp, rng=None, jitter=0.0):
    """(device kernel, NumPy kernel) of the named case with len(cp) + 1 regions; rng: random state means per region."""
    from vidp_amd import kernels as K
    gks = [child(name, K, K, i) for i in range(len(cp) + 1)]
    oks = [child(name, np_kernels, E, i) for i in range(len(cp) + 1)]
    if rng is not None:
        for g, o in zip(gks, oks):
            set_means(g, o, rng)
    return K.PiecewiseKernel(gks, cp, jitter=jitter), PW.PiecewiseKernel(oks, cp, jitter=jitter)


def ssm_grids(rng):
    """Three grids of T = 28 points and 3 change points (4 regions) such that, with 5-node segments (nodes 5 s .. 5 s + 4):
      chain 0: c0 strictly inside segment 0 (between nodes 2 and 3); c1 = t[11] = t[12] exactly, a zero gap on the tie; c2 inside the
               transition 19 -> 20, which crosses a segment boundary; one gap of several periods
      chain 1: starts after c0 (region 0 is never entered); c1 and c2 both between nodes 13 and 14, so region 2 is skipped
      chain 2: starts on c0 exactly; c2 on node 27, the last point of the ragged last segment (nodes 25 .. 27)
    """
    gaps = 0.05 + rng.exponential(0.3, size=(3, 27))
    gaps[0, 11], gaps[0, 22] = 0.0, 7.3
    t = np.concatenate([np.zeros((3, 1)), np.cumsum(gaps, axis=-1)], axis=-1)
    cp = np.array([0.5 * (t[0, 2] + t[0, 3]), t[0, 11], t[0, 19] + 0.25 * gaps[0, 19]])
    assert t[0, 12] == t[0, 11] == cp[1]
    # chain 1: first point after c0, nodes 13 and 14 around (c1, c2)
    lo, hi = cp[0] + 0.01, cp[1] - 0.01
    t[1, :14] = np.linspace(lo, hi, 14)
    t[1, 14:] = cp[2] + 0.01 + np.concatenate([[0.0], np.cumsum(gaps[1, 14:])])
    # chain 2: from c0 to c2
    t[2] = cp[0] + (cp[2] - cp[0]) * np.sort(np.concatenate([[0.0, 1.0], rng.uniform(0.02, 0.98, size=26)]))
    t[2, -1] = cp[2]
    assert (np.diff(t, axis=-1) >= 0).all() and t[1, 0] > cp[0] and t[1, 13] < cp[1] and t[1, 14] > cp[2] and t[2, 0] == cp[0]
    return t, cp


SSM_CASES = [("m12", 1), ("ho", 2), ("m52", 3), ("m32ho", 4), ("m52_m12ho", 5), ("hom32ho", 8)]


@pytest.mark.parametrize("name,d", SSM_CASES)
@pytest.mark.parametrize("jitter", [0.0, 1e-6])
@pytest.mark.parametrize("batch_shape", [(), (3,)], ids=["b0", "b3"])
def test_piecewise_ssm_matches_numpy(amd, rng, name, d, jitter, batch_shape):
    """mfgm_packed_piecewise_ssm against np_piecewise: A, b, chol Q chol Q^T and the initial covariance within 1e-12 of their scale
    (max |Pinf| over the regions for the covariances), the initial mean exactly zero; default partition and 5-node segments."""
    from vidp_amd.packed import Plan
    t, cp = ssm_grids(rng)
    t = t if batch_shape else t[0]
    gk, ok = piecewise(name, cp, rng, jitter)
    assert gk.state_dim == ok.state_dim == d
    _, oP0, oA, ob, oQ = ok.ssm_parameters(t)
    scale = max(np.abs(k.steady_state_covariance()).max() for k in ok.kernels)
    regions = ok.region(t[..., :-1])
    assert set(regions.reshape(-1)) == {0, 1, 2, 3} and (not batch_shape or 2 not in regions[1])
    B = int(np.prod(batch_shape))
    for plan in (None, Plan(B, 28, d, R0=5, device="cuda")):
        g = gk.state_space_model(dev(t), plan=plan)
        assert tuple(g.batch_shape) == batch_shape
        np.testing.assert_allclose(host(g.state_transitions), oA, rtol=0, atol=1e-12 * max(1.0, np.abs(oA).max()))
        np.testing.assert_allclose(host(g.state_offsets), ob, rtol=0, atol=1e-12 * max(1.0, np.abs(ob).max()))
        c = host(g.cholesky_process_covariances)
        np.testing.assert_allclose(c @ np.swapaxes(c, -1, -2), oQ, rtol=0, atol=1e-12 * scale)
        c0 = host(g.cholesky_initial_covariance)
        np.testing.assert_allclose(c0 @ np.swapaxes(c0, -1, -2), oP0, rtol=0, atol=1e-12 * scale)
        np.testing.assert_array_equal(host(g.initial_mean), np.zeros(batch_shape + (d,)))
        if jitter == 0.0:
            zero_gap = np.diff(t, axis=-1) == 0.0
            assert (c[zero_gap] == 0).all()            # Q of a zero gap is exactly zero and stays zero
            if name == "ho":
                assert (c == 0).all()                  # the noise-free kernel's Q is exactly zero in every region
    H = host(gk.generate_emission_model(dev(t)).emission_matrix)
    np.testing.assert_array_equal(H, ok.emission_matrix(t))


@pytest.mark.parametrize("name,d", [("d12", 12), ("m52_m12ho", 5)])
def test_torch_route_matches_numpy(amd, rng, monkeypatch, name, d):
    """The region-selected torch closed forms -- the route of state dimensions above 8 (here d = 12, on the wide sweeps' plan) and, forced
    by VIDP_PIECEWISE_TORCH=1, of any kernel -- against np_piecewise at the tolerances of the HIP route."""
    monkeypatch.setenv("VIDP_PIECEWISE_TORCH", "1")
    t, cp = ssm_grids(rng)
    gk, ok = piecewise(name, cp, rng, 1e-6)
    assert gk.state_dim == d
    _, oP0, oA, ob, oQ = ok.ssm_parameters(t)
    scale = max(np.abs(k.steady_state_covariance()).max() for k in ok.kernels)
    g = gk.state_space_model(dev(t))
    np.testing.assert_allclose(host(g.state_transitions), oA, rtol=0, atol=1e-12 * max(1.0, np.abs(oA).max()))
    np.testing.assert_allclose(host(g.state_offsets), ob, rtol=0, atol=1e-12 * max(1.0, np.abs(ob).max()))
    c = host(g.cholesky_process_covariances)
    np.testing.assert_allclose(c @ np.swapaxes(c, -1, -2), oQ, rtol=0, atol=1e-12 * scale)
    c0 = host(g.cholesky_initial_covariance)
    np.testing.assert_allclose(c0 @ np.swapaxes(c0, -1, -2), oP0, rtol=0, atol=1e-12 * scale)
    np.testing.assert_array_equal(host(g.initial_mean), np.zeros((3, d)))


def unpacked(plan, packed):
    from vidp_amd._lib import FULL, TRI, VEC
    A, off, chol = packed
    return plan.unpack(FULL, A, plan.T - 1), plan.unpack(VEC, off), plan.unpack(TRI, chol)


@pytest.mark.parametrize("nregion", [1, 4])
def test_identical_regions_equal_the_stationary_entry_point(amd, rng, nregion):
    """One region, or four regions of the same parameters: what mfgm_packed_kernel_ssm gives on the same terms, apart from the initial
    mean, within 1e-12 of max |Pinf|."""
    from vidp_amd import kernels as K
    from vidp_amd.packed import Plan
    t, cp = ssm_grids(rng)
    means = [rng.normal(size=n) for n in (3, 2)]

    def twin():
        k = child("m52_m12ho", K, K, 1)
        for c, m in zip(k.kernels, means):
            c.set_state_mean(m)
        return k
    pk = K.PiecewiseKernel([twin() for _ in range(nregion)], cp[:nregion - 1], jitter=1e-9)
    k = twin()
    k.jitter = 1e-9                                     # the stationary twin carries the jitter itself
    plan = Plan(3, 28, k.state_dim, R0=5, device="cuda")
    tt = dev(t)
    a = unpacked(plan, plan.kernel_ssm(k._terms_struct(), (tt[:, 1:] - tt[:, :-1]).contiguous()))
    pw, tab = pk._terms_struct(tt.device)
    b = unpacked(plan, plan.piecewise_ssm(pw, tt))
    plan.check_info()
    scale = float(k.steady_state_covariance.abs().max())
    np.testing.assert_allclose(host(b[0]), host(a[0]), rtol=0, atol=1e-12)
    np.testing.assert_allclose(host(b[2]), host(a[2]), rtol=0, atol=1e-12 * scale)
    np.testing.assert_allclose(host(b[1][:, 1:]), host(a[1][:, 1:]), rtol=0, atol=1e-12 * max(1.0, float(a[1].abs().max())))
    assert (host(b[1][:, 0]) == 0).all() and (host(a[1][:, 0]) != 0).all()


def test_argument_checks(amd):
    """mfgm_packed_piecewise_ssm returns 1 (ValueError) for nregion < 1, a null table and a plan of another state dimension."""
    import torch
    from vidp_amd import kernels as K
    from vidp_amd.packed import Plan
    pk = K.PiecewiseKernel([K.Matern32(1.0, 1.0), K.Matern32(2.0, 1.0)], [0.5])
    t = torch.linspace(0.0, 1.0, 6, dtype=torch.float64, device="cuda")[None]
    plan = Plan(1, 6, 2, device="cuda")
    pw, tab = pk._terms_struct(t.device)
    plan.piecewise_ssm(pw, t)
    plan.check_info()
    for field, value in (("nregion", 0), ("change_points", None), ("rate", None), ("var", None), ("mean", None)):
        pw, tab = pk._terms_struct(t.device)
        setattr(pw, field, value)
        with pytest.raises(ValueError, match="mfgm_packed_piecewise_ssm"):
            plan.piecewise_ssm(pw, t)
    pw, tab = pk._terms_struct(t.device)
    with pytest.raises(ValueError, match="mfgm_packed_piecewise_ssm"):
        Plan(1, 6, 3, device="cuda").piecewise_ssm(pw, t)
    pw.nregion, pw.change_points = 1, None               # one region needs no change-point table
    plan.piecewise_ssm(pw, t)
    plan.check_info()


def test_reference_stitched_case(amd):
    """The reference's two-region Matern32 case with the change point at -1e-5: the marginals on the device equal those of the two
    separately built chains stitched at 0 (NumPy), atol 1e-10."""
    from vidp_amd import kernels as K
    ks, xs, x = PW.stitched_case()
    pk = K.PiecewiseKernel([K.Matern32(k.lengthscale, k.variance) for k in ks], [-1e-5])
    mu, cov = pk.state_space_model(dev(x)).marginals
    np.testing.assert_allclose(host(cov), PW.marginal_covariances(*PW.stitched_parameters(ks, xs)), rtol=0, atol=1e-10)
    np.testing.assert_allclose(host(mu), 0.0, rtol=0, atol=1e-10)


def test_not_positive_definite_q_raises(amd):
    """Regions of Sum(Matern12, HarmonicOscillator) without a jitter: Q = diag(q, 0, 0) is neither positive definite nor zero."""
    t = dev(np.linspace(0.0, 3.0, 30))
    gk, _ = piecewise("m12_ho", [1.0, 2.0])
    with pytest.raises(ArithmeticError, match="set a jitter"):
        gk.state_space_model(t)
    gk.jitter = 1e-6
    gk.state_space_model(t)


def test_gpr_log_likelihood_equals_the_dense_gp(amd, rng):
    """GaussianProcessRegression.log_likelihood() on a 3-region Matern32 prior (T = 60, gaps >= 0.03: Q = Pinf - A Pinf A^T loses digits
    to cancellation at tiny gaps, in any SSM) equals the dense Gaussian log density of the NumPy SSM's f covariance plus noise at rtol
    1e-9."""
    from vidp_amd import kernels as K
    from vidp_amd.variational_cvi import GaussianProcessRegression
    t, y, cp, prm, noise = PW.gpr_case(rng)
    gk = K.PiecewiseKernel([K.Matern32(*p) for p in prm], cp)
    ok = PW.PiecewiseKernel([np_kernels.Matern32(*p) for p in prm], cp)
    g = GaussianProcessRegression((dev(t), dev(y)), gk, chol_obs_covariance=dev(np.array([[np.sqrt(noise)]])))
    dense = PW.dense_logml(PW.f_covariance(ok, t) + noise * np.eye(t.size), y[:, 0])
    np.testing.assert_allclose(float(g.log_likelihood()), dense, rtol=1e-9)
    assert len(set(ok.region(t))) == 3


def test_prediction_across_change_points(amd, rng, monkeypatch):
    """predict_f at 25 new unsorted times (before the first and after the last training point, inside every region) equals dense
    conditioning of the NumPy SSM built on the union grid at 1e-8, on the fused and on the generic route.  Every change point lies on
    a training point, so no transition of either grid crosses one; otherwise the two grids define different priors (the reference's
    documented caveat).  sample_f is reproducible."""
    from vidp_amd import kernels as K
    from vidp_amd.variational_cvi import GaussianProcessRegression
    t, y, cp, prm, noise, tn = PW.predict_case(rng)
    gk = K.PiecewiseKernel([K.Matern32(*p) for p in prm], cp)
    ok = PW.PiecewiseKernel([np_kernels.Matern32(*p) for p in prm], cp)
    om, ov = PW.dense_predict(ok, t, y, noise, tn)
    g = GaussianProcessRegression((dev(t), dev(y)), gk, chol_obs_covariance=dev(np.array([[np.sqrt(noise)]])))
    for fused in ("1", "0"):
        monkeypatch.setenv("VIDP_FUSED_PREDICT", fused)
        mu, var = g.posterior.predict_f(dev(tn))
        np.testing.assert_allclose(host(mu).reshape(-1), om, rtol=1e-8, atol=1e-8)
        np.testing.assert_allclose(host(var).reshape(-1), ov, rtol=1e-8, atol=1e-8)
    s1 = host(g.posterior.sample_f(dev(tn), (3,), seed=5))
    s2 = host(g.posterior.sample_f(dev(tn), (3,), seed=5))
    np.testing.assert_array_equal(s1, s2)
    assert np.isfinite(s1).all() and s1.shape == (3, 25, 1)


def _cls_data(rng, t, which):
    f = 1.5 * np.sin(3 * t)
    if which == "bernoulli":
        return (f + 0.5 * rng.normal(size=t.size) > 0).astype(np.float64)[:, None]
    return rng.poisson(np.exp(f)).astype(np.float64)[:, None]


# Matern52 (lengthscale, variance) per region of the model tests.  Their grids keep every gap above a quarter of every lengthscale
# (linspace(0, 8, 40): gaps 0.205, lengthscales <= 0.9): Q = Pinf - A Pinf A^T cancels like (gap / lengthscale)^5 in its smallest
# direction, and the NumPy reference evaluated in two algebraically equal operation orders differs from itself by 3e-9 on
# linspace(0, 4, 40) with a lengthscale of 1.4 -- above the 1e-9 these tests hold -- and by 2e-12 on the grid used here.
M52 = [(0.6, 1.2), (0.9, 0.5), (0.35, 2.0)]


def test_cvi_gp_bernoulli_against_numpy(amd, rng):
    """CVIGaussianProcess with a Bernoulli likelihood on a 3-region Matern52 prior (T = 40, d = 3): after each of 3 update_sites() the
    sites, elbo() and classic_elbo() agree with oracle/np_models.CVIGaussianProcess driven by the NumPy SSM (the tolerances of
    test_cvi_gp_bernoulli_against_oracle)."""
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Bernoulli
    from vidp_amd.variational_cvi import CVIGaussianProcess
    t = np.linspace(0.0, 8.0, 40)
    y = _cls_data(rng, t, "bernoulli")
    cp = [2.6, t[25]]
    g = CVIGaussianProcess((dev(t), dev(y)), K.PiecewiseKernel([K.Matern52(*p) for p in M52], cp), Bernoulli(), learning_rate=0.5)
    o = np_models.CVIGaussianProcess(t, y, PW.PiecewiseKernel([np_kernels.Matern52(*p) for p in M52], cp), np_lik.Bernoulli(),
                                     learning_rate=0.5)
    for _ in range(3):
        g.update_sites()
        o.update_sites()
        np.testing.assert_allclose(host(g.sites.nat1), o.nat1, rtol=1e-9, atol=1e-9 * np.abs(o.nat1).max())
        np.testing.assert_allclose(host(g.sites.nat2), o.nat2, rtol=1e-9, atol=1e-9 * np.abs(o.nat2).max())
        np.testing.assert_allclose(float(g.elbo()), o.elbo(), rtol=1e-9)
        np.testing.assert_allclose(float(g.classic_elbo()), o.classic_elbo(), rtol=1e-9)


@pytest.mark.parametrize("route", ["fused", "generic"])
def test_sparse_cvi_poisson_against_numpy(amd, rng, monkeypatch, route):
    """SparseCVIGaussianProcess with a Poisson likelihood on a 3-region Matern52 prior, 8 inducing points, 50 data points, the change
    points on inducing points: sites and classic_elbo over 3 steps against the NumPy model with time-aware conditionals, on the fused
    sorted-data route and on the generic route (the tolerances of test_sparse_cvi_poisson_against_oracle)."""
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Poisson
    from vidp_amd.sparse_variational_cvi import SparseCVIGaussianProcess
    if route == "generic":
        monkeypatch.setenv("VIDP_FUSED_SPARSE", "0")
    t = np.linspace(0.0, 1.0, 50)
    y = _cls_data(rng, t, "poisson")
    z = np.linspace(-0.1, 1.1, 8)
    cp = [z[2], z[5]]
    g = SparseCVIGaussianProcess(K.PiecewiseKernel([K.Matern52(*p) for p in M52], cp, jitter=1e-9), dev(z), Poisson(1.3),
                                 learning_rate=0.6)
    o = PW.SparseCVIGaussianProcess(PW.PiecewiseKernel([np_kernels.Matern52(*p) for p in M52], cp, jitter=1e-9), z, np_lik.Poisson(1.3),
                                    learning_rate=0.6)
    data = (dev(t), dev(y))
    assert (g._data(data) is None) == (route == "generic")
    for _ in range(3):
        g.update_sites(data)
        o.update_sites(t, y)
        np.testing.assert_allclose(host(g.nat1), o.nat1, rtol=1e-9, atol=1e-9 * np.abs(o.nat1).max())
        np.testing.assert_allclose(host(g.nat2), o.nat2, rtol=1e-9, atol=1e-9 * np.abs(o.nat2).max())
    np.testing.assert_allclose(float(g.classic_elbo(data)), o.classic_elbo(t, y), rtol=1e-9)


def test_power_ep_against_numpy(amd, rng):
    """PowerExpectationPropagation (Bernoulli, alpha = 0.5) on the 3-region Matern52 prior follows the dense tests/np_pep model driven
    by the NumPy SSM over 3 full sweeps (the 1e-9 of test_model_against_numpy)."""
    from tests import np_pep
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Bernoulli, PEPScalarLikelihood
    from vidp_amd.pep import PowerExpectationPropagation
    t = np.linspace(0.0, 8.0, 40)
    y = _cls_data(rng, t, "bernoulli")
    cp = [2.6, t[25]]
    g = PowerExpectationPropagation((dev(t), dev(y)), K.PiecewiseKernel([K.Matern52(*p) for p in M52], cp), PEPScalarLikelihood(Bernoulli(1e-3)),
                                    learning_rate=0.5, alpha=0.5)
    o = np_pep.PowerExpectationPropagation(t, y[:, 0], PW.PiecewiseKernel([np_kernels.Matern52(*p) for p in M52], cp), "bernoulli", 1e-3,
                                           learning_rate=0.5, alpha=0.5)
    idx = np.arange(40).reshape(-1, 1)
    for _ in range(3):
        g.update_sites(idx)
        o.update_sites(idx)
        for a, b in ((g.sites.nat1[:, 0], o.nat1), (g.sites.nat2[:, 0, 0], o.nat2)):
            np.testing.assert_allclose(host(a), b, rtol=1e-9, atol=1e-9 * np.abs(b).max())
        np.testing.assert_allclose(float(g.elbo()), o.elbo(), rtol=1e-9)


def test_hyperparameter_tape_gives_per_region_gradients(amd, rng):
    """d classic_elbo / d (lengthscale, variance) of region 1 through classic_elbo_tape_hyper (sites held fixed) equals central
    differences of classic_elbo() on rebuilt kernels with the same sites at rtol 1e-5 (T = 30); region 2 lies between two consecutive
    points -- it holds no time point and no left end -- and its gradient is exactly 0."""
    import torch
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Bernoulli
    from vidp_amd.variational_cvi import CVIGaussianProcess
    t = np.linspace(0.0, 5.0, 30) + 0.05 * rng.uniform(-1, 1, size=30)
    y = _cls_data(rng, t, "bernoulli")
    mid = 0.5 * (t[19] + t[20])
    cp = [t[9], mid - 0.01, mid + 0.01]
    hyp = [[0.9, 1.1], [0.5, 1.7], [2.0, 0.3], [1.3, 0.8]]          # Matern32 (lengthscale, variance) per region

    def model(h):
        return CVIGaussianProcess((dev(t), dev(y)), K.PiecewiseKernel([K.Matern32(*p) for p in h], cp), Bernoulli(), learning_rate=0.5)
    g = model(hyp)
    for _ in range(2):
        g.update_sites()
    nat1, nat2 = g.sites.nat1.clone(), g.sites.nat2.clone()
    elbo, leaves = g.classic_elbo_tape_hyper()
    assert len(leaves) == 4
    np.testing.assert_allclose(float(elbo.detach()), float(g.classic_elbo()), rtol=1e-8)
    names = [(1, "lengthscale", 0), (1, "variance", 1), (2, "lengthscale", 0), (2, "variance", 1)]
    grads = torch.autograd.grad(elbo, [leaves[r][n] for r, n, _ in names])

    def at(r, i, e):
        h = [list(p) for p in hyp]
        h[r][i] += e
        m = model(h)
        m.sites.nat1.copy_(nat1)
        m.sites.nat2.copy_(nat2)
        return float(m.classic_elbo())
    e = 1e-3
    for (r, n, i), gr in zip(names[:2], grads[:2]):
        fd = (8 * (at(r, i, e) - at(r, i, -e)) - (at(r, i, 2 * e) - at(r, i, -2 * e))) / (12 * e)
        np.testing.assert_allclose(float(gr), fd, rtol=1e-5)
    assert float(grads[2]) == 0.0 and float(grads[3]) == 0.0


def test_notebook_configuration_runs(amd, rng):
    """The configuration of the reference's piecewise-kernel notebook, scaled down: Matern52, 5 change points, per-region state means,
    through GaussianProcessRegression (its log-likelihood against the dense Gaussian density with the SSM's prior mean, rtol 1e-9)
    and SparseCVIGaussianProcess (a finite ELBO that the site updates raise)."""
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Gaussian
    from vidp_amd.sparse_variational_cvi import SparseCVIGaussianProcess
    from vidp_amd.variational_cvi import GaussianProcessRegression
    t = np.cumsum(0.05 + rng.exponential(0.07, size=120))      # gaps >= 0.05 for lengthscales >= 0.3: see the GPR test
    z = t[::8].copy()
    cp = z[[2, 5, 7, 10, 12]]
    ls = [0.4, 1.0, 0.3, 0.6, 1.5, 0.5]
    means = rng.normal(size=(6, 3)) * [1.0, 0.1, 0.01]
    y = np.sin(t * np.array(ls)[np.searchsorted(cp, t, side="right")] * 6.0)[:, None] + 0.1 * rng.normal(size=(120, 1))

    def mk(m):
        ks = [m.Matern52(l, 1.0) for l in ls]
        for k, mean in zip(ks, means):
            k._state_mean = mean
        return ks
    gk, ok = K.PiecewiseKernel(mk(K), cp, jitter=1e-9), PW.PiecewiseKernel(mk(np_kernels), cp, jitter=1e-9)
    noise = 0.05
    g = GaussianProcessRegression((dev(t), dev(y)), gk, chol_obs_covariance=dev(np.array([[np.sqrt(noise)]])))
    dense = PW.dense_logml(PW.f_covariance(ok, t) + noise * np.eye(t.size), y[:, 0] - PW.f_mean(ok, t))
    np.testing.assert_allclose(float(g.log_likelihood()), dense, rtol=1e-9)
    s = SparseCVIGaussianProcess(gk, dev(z), Gaussian(noise), learning_rate=0.8)
    data = (dev(t), dev(y))
    e0 = float(s.classic_elbo(data))
    for _ in range(4):
        s.update_sites(data)
    e1 = float(s.classic_elbo(data))
    assert np.isfinite(e0) and np.isfinite(e1) and e1 > e0
