"""
GPU tests of sparse Power Expectation Propagation (vidp_amd.sparse_pep.SparsePowerExpectationPropagation; kernels
mfgm_sparse_pep_sites / mfgm_sparse_pep_sites_q, csrc/mfgm_spep.h): the kernel against the NumPy per-interval update of
tests/np_spep.py, null outputs, energy mode and skipped intervals, the native route against the torch route and the dense NumPy model,
the reference's tests seeded from SparseCVIGaussianProcess, the closed-form energy at M = N = 2 000 and a Bernoulli run at config 5's
miniature shape.  fp64.
"""
import ctypes

import numpy as np
import pytest

from oracle import np_kernels, np_models
from tests import np_lik, np_spep

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


def _pack(nat2, d):
    """[M1, 2d, 2d] -> quadrant-packed [M1, d (d + 1) + d^2] (include/mfgm.h)."""
    i, j = np.tril_indices(d)
    return np.concatenate([nat2[:, i, j], nat2[:, d:, :d].reshape(len(nat2), -1), nat2[:, d + i, d + j]], axis=1)


def _case(rng, d, kind, alpha, M1):
    """Random well-conditioned pair marginals given as chain blocks (M = M1 - 1 states), sites with proper cavities, 0-5 points per
    interval with projections scaled so that the cavity variances of f lie around 0.03 - 1."""
    n, M = 2 * d, M1 - 1
    A = rng.normal(size=(M1, n, n)) / np.sqrt(n)
    S = A @ A.transpose(0, 2, 1) + 0.5 * np.eye(n)
    # consistent chain blocks: interval m = (state m-1, state m); take Sig_m from the lower-right block of pair m and rebuild pair m+1's
    # upper-left block from it, so that consecutive pairs share their common state
    Sig = S[:M, d:, d:].copy()
    Sub = np.zeros((M, d, d))
    Sub[:M - 1] = 0.3 * S[1:M, d:, :d]
    P0 = S[M, d:, d:].copy()
    mu = rng.normal(size=(M, d))
    pm = 0.1 * rng.normal(size=d)
    pair = np.zeros((M1, n, n))
    pmu = np.zeros((M1, n))
    for m in range(M1):
        lo, hi = (P0, pm) if m == 0 else (Sig[m - 1], mu[m - 1]), (P0, pm) if m == M else (Sig[m], mu[m])
        pair[m, :d, :d], pair[m, d:, d:] = lo[0], hi[0]
        if 0 < m < M:
            pair[m, d:, :d], pair[m, :d, d:] = Sub[m - 1], Sub[m - 1].T
        pmu[m] = np.concatenate([lo[1], hi[1]])
    assert np.linalg.eigvalsh(pair).min() > 0.05
    cnt = rng.integers(0, 6, size=M1)
    cnt[:3] = (5, 0, 1)
    seg = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    N = int(cnt.sum())
    w = rng.normal(size=(N, n)) * (0.6 / np.sqrt(n))
    c = rng.uniform(0.0, 0.2, size=N)
    if kind == "bernoulli":
        y = rng.choice([0.0, 1.0], size=N)
    elif kind == "poisson":
        y = rng.poisson(1.5, size=N).astype(np.float64)
        pmu *= 0.5
        mu *= 0.5
        pm *= 0.5
    else:
        y = rng.normal(size=N)
    # sites with proper cavities whatever n_m: nat2 = -1/2 C R diag(u) R^T C^T with Lam = C C^T, R orthogonal, u in (-0.4, 0.9), so that
    # Lam + 2 beta nat2 = C R diag(1 - beta u) R^T C^T is positive definite for every beta <= 1
    C = np.linalg.cholesky(np.linalg.inv(pair))
    R = np.linalg.qr(rng.normal(size=(M1, n, n)))[0]
    CR = C @ R
    nat2 = -0.5 * (CR * rng.uniform(-0.4, 0.9, size=(M1, 1, n))) @ CR.transpose(0, 2, 1)
    nat2 = 0.5 * (nat2 + nat2.transpose(0, 2, 1))
    nat1 = 0.3 * rng.normal(size=(M1, n))
    return dict(d=d, M=M, seg=seg, w=w, c=c, y=y, Sig=Sig, Sub=Sub, mu=mu, P0=P0, pm=pm, pair=pair, pmu=pmu, nat1=nat1, nat2=nat2,
                ln=rng.normal(size=M1), cnt=cnt)


def spep_sites(amd, cs, kind, param, alpha, lr, packed=False, want_e=True, want_ln=True, want_sk=True):
    """Direct call of mfgm_sparse_pep_sites[_q] on device copies; returns host (nat1, nat2 (dense or packed), lnorm, e, skipped)."""
    import torch
    from vidp_amd.packed import _ptr, _stream
    d, M = cs["d"], cs["M"]
    keep = [dev(cs["seg"], np.int32), dev(cs["w"] if len(cs["w"]) else np.zeros((1, 2 * d))), dev(cs["c"] if len(cs["c"]) else np.zeros(1)),
            dev(cs["pm"]), dev(cs["P0"]), dev(cs["y"] if len(cs["y"]) else np.zeros(1))]
    sd = amd._lib.SparseData()
    sd.M, sd.d, sd.N, sd.m_lo, sd.m_hi = M, d, len(cs["y"]), 0, 0
    sd.seg, sd.w, sd.c, sd.prior_mean, sd.prior_cov = (t.data_ptr() for t in keep[:5])
    b = [dev(cs["mu"]), dev(cs["Sig"]), dev(cs["Sub"]), dev(cs["nat1"]), dev(_pack(cs["nat2"], d) if packed else cs["nat2"]), dev(cs["ln"])]
    e = torch.full((M + 1,), 7.0, dtype=torch.float64, device="cuda")
    sk = torch.zeros(1, dtype=torch.int32, device="cuda")
    lib = amd._lib.load()
    fn = lib.mfgm_sparse_pep_sites_q if packed else lib.mfgm_sparse_pep_sites
    amd._lib.check(fn(ctypes.byref(sd), kind, _ptr(keep[5]), param, alpha, lr, _ptr(b[0]), _ptr(b[1]), _ptr(b[2]), _ptr(b[3]), _ptr(b[4]),
                      _ptr(b[5]) if want_ln else None, _ptr(e) if want_e else None, _ptr(sk) if want_sk else None, _stream()),
                   "mfgm_sparse_pep_sites")
    torch.cuda.synchronize()
    return host(b[3]), host(b[4]), host(b[5]), host(e), int(sk.item())


def _np_update(cs, kind, alpha, lr, route, scales=False):
    return np_spep.interval_update(kind, cs["seg"], cs["w"], cs["c"], cs["y"], cs["pmu"], cs["pair"], cs["nat1"], cs["nat2"], cs["ln"],
                                   KINDS[kind][1], alpha, lr, route, scales=scales)


@pytest.mark.parametrize("alpha", [0.5, 0.9, 1.0])
@pytest.mark.parametrize("kind", ["gaussian", "bernoulli", "poisson"])
@pytest.mark.parametrize("d", [1, 2, 3, 6, 8, 16, 32])
def test_kernel_matches_numpy(amd, rng, d, kind, alpha):
    """mfgm_sparse_pep_sites and its _q twin over 10 000 intervals with 0 - 5 points each (2 000 at d = 32, whose [M + 1, 64, 64] NumPy
    batches would otherwise take gigabytes; d = 32 fits the 64 KB of LDS a workgroup may ask for, so no d falls back), lr = 0.7,
    against np_spep.interval_update.  Bound: 10 x the largest disagreement of the NumPy update's two routes (explicit inverse, Cholesky
    solve) on the same inputs, relative to the sum of absolute terms of each output, floored at 1e-12.  Measured on an MI355X: the
    NumPy routes disagree by at most 1.4e-14 of the scale (so the bound is the floor), the kernel by at most 1.7e-14."""
    k, param = KINDS[kind]
    cs = _case(rng, d, kind, alpha, 2000 if d == 32 else 10000)
    a = _np_update(cs, kind, alpha, 0.7, "inverse", scales=True)
    b = _np_update(cs, kind, alpha, 0.7, "cholesky")
    assert a[4] == 0 and b[4] == 0
    sc = a[5]
    routes = max(float(np.max(np.abs(x - y) / s)) for x, y, s in zip(a[:4], b[:4], (sc[0], sc[1], sc[2], sc[3])))
    bound = max(10.0 * routes, 1e-12)
    g = spep_sites(amd, cs, k, param, alpha, 0.7)
    q = spep_sites(amd, cs, k, param, alpha, 0.7, packed=True)
    assert g[4] == 0 and q[4] == 0
    errs = [float(np.max(np.abs(x - y) / s)) for x, y, s in zip(g[:4], a[:4], (sc[0], sc[1], sc[2], sc[3]))]
    print(f"spep d={d} {kind} alpha={alpha}: numpy routes {routes:.2e} bound {bound:.2e} kernel {max(errs):.2e}")
    assert max(errs) <= bound, (errs, bound)
    # the packed twin: the same sites (its lower triangle), log_norm and e
    np.testing.assert_allclose(q[1], _pack(g[1], d), rtol=1e-13, atol=1e-13 * np.abs(g[1]).max())
    for x, y in ((q[0], g[0]), (q[2], g[2]), (q[3], g[3])):
        np.testing.assert_allclose(x, y, rtol=1e-13, atol=1e-13)
    # the dense form keeps the site symmetric
    np.testing.assert_allclose(g[1], g[1].transpose(0, 2, 1), rtol=1e-13, atol=1e-14 * np.abs(g[1]).max())


@pytest.mark.parametrize("packed", [False, True])
def test_null_outputs_energy_mode_and_skipped_intervals(amd, rng, packed):
    """lr = 0 writes e alone; null lnorm / e_out / skipped are left alone; an interval whose Lam_c is indefinite keeps site and
    lnorm bit for bit, gets e = NaN and adds its n_m points to the counter, its neighbours update; argument errors return 1."""
    d, kind, alpha = 3, "bernoulli", 0.9
    k, param = KINDS[kind]
    cs = _case(rng, d, kind, alpha, 500)
    n2 = lambda a: _pack(a, d) if packed else a
    g = spep_sites(amd, cs, k, param, alpha, 0.0, packed=packed)
    np.testing.assert_array_equal(g[0], cs["nat1"])
    np.testing.assert_array_equal(g[1], n2(cs["nat2"]))
    np.testing.assert_array_equal(g[2], cs["ln"])
    want = _np_update(cs, kind, alpha, 0.0, "inverse")
    np.testing.assert_allclose(g[3], want[3], rtol=1e-10, atol=1e-10)
    g = spep_sites(amd, cs, k, param, alpha, 0.5, packed=packed, want_e=False, want_ln=False, want_sk=False)
    np.testing.assert_array_equal(g[2], cs["ln"])
    assert np.all(g[3] == 7.0) and g[4] == 0
    np.testing.assert_allclose(g[1], n2(_np_update(cs, kind, alpha, 0.5, "inverse")[1]), rtol=1e-10, atol=1e-12)
    # improper cavities at intervals with data, and one at an interval without (which is not a cavity at all: it updates)
    bad = [m for m in rng.choice(500, size=40, replace=False)]
    Lam = np.linalg.inv(cs["pair"])
    for m in bad:
        v = rng.normal(size=2 * d)
        cs["nat2"][m] = -(Lam[m] + 3.0 * np.outer(v, v)) / (2.0 * alpha / max(cs["cnt"][m], 1)) * 1.5
    g = spep_sites(amd, cs, k, param, alpha, 1.0, packed=packed)
    want = _np_update(cs, kind, alpha, 1.0, "inverse")
    skip = [m for m in bad if cs["cnt"][m] > 0]
    assert g[4] == want[4] == int(cs["cnt"][skip].sum()) and len(skip) > 10
    np.testing.assert_array_equal(g[0][skip], cs["nat1"][skip])
    np.testing.assert_array_equal(g[1][skip], n2(cs["nat2"])[skip])
    np.testing.assert_array_equal(g[2][skip], cs["ln"][skip])
    assert np.isnan(g[3][skip]).all() and np.isfinite(np.delete(g[3], skip)).all()
    np.testing.assert_allclose(g[1], n2(want[1]), rtol=1e-9, atol=1e-11 * np.abs(want[1]).max())
    np.testing.assert_allclose(g[2], want[2], rtol=1e-9, atol=1e-9)
    for args in ((9, param, alpha, 0.5), (k, 0.7, alpha, 0.5), (k, param, 0.0, 0.5), (k, param, 1.5, 0.5), (k, param, alpha, 1.5)):
        with pytest.raises(ValueError):
            spep_sites(amd, cs, *args, packed=packed)


def _lik(kind):
    from vidp_amd.likelihoods import Bernoulli, Gaussian, PEPGaussian, PEPScalarLikelihood, Poisson
    return {"gaussian": lambda: PEPGaussian(Gaussian(KINDS["gaussian"][1])), "bernoulli": lambda: PEPScalarLikelihood(Bernoulli(1e-3)),
            "poisson": lambda: PEPScalarLikelihood(Poisson(1.3))}[kind]()


def _ve(kind):
    return {"gaussian": np_models.GaussianLik(KINDS["gaussian"][1]), "bernoulli": np_lik.Bernoulli(1e-3),
            "poisson": np_lik.Poisson(1.3)}[kind].variational_expectations


def _obs(rng, kind, t):
    f = 1.5 * np.sin(0.6 * t)
    if kind == "gaussian":
        return f + np.sqrt(KINDS["gaussian"][1]) * rng.normal(size=t.size)
    if kind == "bernoulli":
        return (f + 0.5 * rng.normal(size=t.size) > 0).astype(np.float64)
    return rng.poisson(np.exp(0.5 * f)).astype(np.float64)


def _config5_kernel(mod, scale=1.0):
    ls = np.exp(np.linspace(np.log(0.05), np.log(2.0), 6))
    return mod.Sum([mod.Matern52(float(l), scale) for l in ls[:4]] + [mod.Matern32(float(l), scale) for l in ls[4:]])


@pytest.mark.parametrize("alpha", [0.5, 1.0])
@pytest.mark.parametrize("kind", ["gaussian", "bernoulli", "poisson"])
@pytest.mark.parametrize("shape", ["d3", "c5"])
def test_native_model_against_torch_route_and_numpy(amd, rng, monkeypatch, shape, kind, alpha):
    """The native route (one launch per update) follows the torch route of the same class (VIDP_FUSED_SPARSE=0) and the dense NumPy
    model over 10 damped steps: Matern-5/2 (d = 3) with several points per interval, empty intervals and points outside the inducing
    points, to 1e-9; config 5 in miniature (its d = 16 kernel, grid spacing 0.1 = 2 of its shortest lengthscales, 2 points per
    inducing state) to 1e-8, the figure of test_sparse_cvi_config5_grid.  Nothing is skipped."""
    from vidp_amd import kernels as K
    from vidp_amd.sparse_pep import SparsePowerExpectationPropagation
    sc = 0.25 if kind == "poisson" else 1.0
    if shape == "d3":
        z = np.linspace(0.0, 6.0, 25)
        t = np.sort(rng.uniform(-0.5, 6.6, size=70))
        t = t[~((t > z[3]) & (t < z[4])) & ~((t > z[11]) & (t < z[12]))]
        kg, ko, tol = K.Matern52(1.0, 1.5 * sc), np_kernels.Matern52(1.0, 1.5 * sc), 1e-9
    else:
        M, dz = 40, 0.1
        z = np.linspace(0, dz * M, M)
        t = np.sort(rng.uniform(0, dz * M, size=2 * M))
        # Poisson: the six components together carry a quarter of a unit prior variance, as the d = 3 model does (at cavity
        # variances ~ 1 the 20-point rule gives zero counts a negative site precision: DESIGN.md section 13)
        kg, ko, tol = _config5_kernel(K, sc if kind != "poisson" else sc / 6.0), _config5_kernel(np_kernels, sc if kind != "poisson" else sc / 6.0), 1e-8
    y = _obs(rng, kind, t)
    data = (dev(t), dev(y[:, None]))
    a = SparsePowerExpectationPropagation(kg, dev(z), _lik(kind), learning_rate=0.5, alpha=alpha)
    assert a._native(a._data(data)) and a._packed == (shape == "c5")
    monkeypatch.setenv("VIDP_FUSED_SPARSE", "0")
    b = SparsePowerExpectationPropagation(kg, dev(z), _lik(kind), learning_rate=0.5, alpha=alpha)
    assert b._data(data) is None
    monkeypatch.delenv("VIDP_FUSED_SPARSE")
    o = np_spep.SparsePowerExpectationPropagation(ko, z, kind, KINDS[kind][1], learning_rate=0.5, alpha=alpha, ve=_ve(kind))
    for _ in range(10):
        a.update_sites(data)
        monkeypatch.setenv("VIDP_FUSED_SPARSE", "0")
        b.update_sites(data)
        eb = float(b.energy(data))
        monkeypatch.delenv("VIDP_FUSED_SPARSE")
        o.update_sites(t, y)
        for x, w1, w2 in ((a.nat1, b.nat1, o.nat1), (a.nat2, b.nat2, o.nat2), (a.log_norm[:, 0], b.log_norm[:, 0], o.log_norm)):
            np.testing.assert_allclose(host(x), host(w1), rtol=tol, atol=tol * np.abs(w2).max())
            np.testing.assert_allclose(host(x), w2, rtol=tol, atol=tol * np.abs(w2).max())
        np.testing.assert_allclose(float(a.energy(data)), eb, rtol=tol)
        np.testing.assert_allclose(float(a.energy(data)), o.energy(t, y), rtol=tol)
        np.testing.assert_allclose(float(a.classic_elbo(data)), o.classic_elbo(t, y), rtol=tol)
    assert a.num_skipped == 0 and b.num_skipped == 0 and o.skipped == 0
    a.dist_p.plan.check_info()


def test_reference_tests_seeded_from_sparse_cvi(amd, rng):
    """The reference's test_optimal_sites / test_log_norm / test_convergence_of_spep: Matern-1/2 (2, 2.25), two points, noise 1,
    z = x + 1e-10, sites seeded from one lr = 1 step of SparseCVIGaussianProcess."""
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Gaussian, PEPScalarLikelihood
    from vidp_amd.sparse_pep import SparsePowerExpectationPropagation
    from vidp_amd.sparse_variational_cvi import SparseCVIGaussianProcess
    x = np.sort(rng.uniform(0.0, 3.0, 2))
    y = rng.normal(size=(2, 1))
    z = x + 1e-10
    data = (dev(x), dev(y))
    llh = np_models.gpr_log_likelihood(x, y, np_kernels.Matern12(2.0, 2.25), 1.0)
    want_ln = -0.5 * y ** 2 - 0.5 * np.log(2.0 * np.pi)

    def seeded():
        sep = SparsePowerExpectationPropagation(K.Matern12(2.0, 2.25), dev(z), PEPScalarLikelihood(Gaussian(1.0)), learning_rate=0.1,
                                                alpha=1.0)
        scvi = SparseCVIGaussianProcess(K.Matern12(2.0, 2.25), dev(z), Gaussian(1.0), learning_rate=1.0)
        scvi.update_sites(data)
        sep.nat1, sep.nat2 = scvi.nat1.clone(), scvi.nat2.clone()
        return sep

    sep = seeded()
    np.testing.assert_array_almost_equal(host(sep.compute_log_norm(data))[:-1, None], want_ln, decimal=4)
    sep.learning_rate = 1.0
    sep.update_sites(data)
    np.testing.assert_array_almost_equal(host(sep.nat1)[:-1, 1:], y, decimal=3)
    np.testing.assert_array_almost_equal(host(sep.nat2)[:-1, 1:, 1:], -0.5 * np.ones((2, 1, 1)), decimal=3)
    np.testing.assert_array_almost_equal(host(sep.log_norm)[:-1], want_ln, decimal=4)
    np.testing.assert_array_almost_equal(float(sep.energy(data)), llh, decimal=4)
    sep = seeded()
    for _ in range(20):
        sep.update_sites(data)
    old1, old2 = host(sep.nat1).copy(), host(sep.nat2).copy()
    sep.update_sites(data)
    np.testing.assert_array_almost_equal(host(sep.nat1), old1)
    np.testing.assert_array_almost_equal(host(sep.nat2), old2)
    np.testing.assert_array_almost_equal(float(sep.energy(data)), llh, decimal=4)
    assert sep.num_skipped == 0


@pytest.mark.parametrize("alpha", [0.5, 1.0])
def test_known_answer_at_size(amd, rng, alpha):
    """M = N = 2 000, Matern-5/2, inducing points 0.2 lengthscales apart, one Gaussian observation in the middle of every interval
    between inducing points and one before the first: the converged energy equals the closed form
    log N(y; 0, W K_uu W^T + diag(alpha c + s^2)) - (1 - alpha) / (2 alpha) sum_i log(1 + alpha c_i / s^2), evaluated densely in
    float64 on the host, to rtol 1e-8."""
    from vidp_amd import kernels as K
    from vidp_amd.sparse_pep import SparsePowerExpectationPropagation
    M, s2 = 2000, KINDS["gaussian"][1]
    z = 0.2 * np.arange(M)
    t = z - 0.1
    y = 1.5 * np.sin(0.03 * t) + np.sqrt(s2) * rng.normal(size=M)
    g = SparsePowerExpectationPropagation(K.Matern52(1.0, 1.5), dev(z), _lik("gaussian"), learning_rate=1.0, alpha=alpha)
    data = (dev(t), dev(y[:, None]))
    assert g._native(g._data(data))
    for _ in range(2 if alpha == 1.0 else 60):
        g.update_sites(data)
    ko = np_kernels.Matern52(1.0, 1.5)
    seg, w, c = np_spep.data_terms(ko, z, t)
    d = 3
    W = np.zeros((M, (M + 2) * d))
    for i in range(M):
        W[i, i * d:(i + 2) * d] = w[i]
    from tests import np_pep
    Kuu = np.linalg.inv(np_pep.dense_precision(ko.state_space_model(z)))
    want = np_spep.gaussian_closed_form(Kuu, W[:, d:-d], c, y, s2, alpha)
    got = float(g.energy(data))
    print(f"known answer alpha={alpha}: energy {got!r} closed form {want!r} rel {abs(got - want) / abs(want):.2e}")
    np.testing.assert_allclose(got, want, rtol=1e-8)
    assert g.num_skipped == 0
    g.dist_p.plan.check_info()


def test_bernoulli_run_at_config5_miniature(amd, rng):
    """20 native steps with Bernoulli data at config 5's miniature shape (d = 16, 120 inducing states 0.1 apart, 2 observations per
    state): every site finite, classic_elbo finite, nothing skipped."""
    import torch
    from vidp_amd import kernels as K
    from vidp_amd.sparse_pep import SparsePowerExpectationPropagation
    M, dz = 120, 0.1
    z = np.linspace(0, dz * M, M)
    t = np.sort(rng.uniform(0, dz * M, size=2 * M))
    y = (np.sin(3 * t) + 0.5 * rng.normal(size=t.size) > 0).astype(np.float64)
    g = SparsePowerExpectationPropagation(_config5_kernel(K), dev(z), _lik("bernoulli"), learning_rate=0.5, alpha=0.9)
    data = (dev(t), dev(y[:, None]))
    assert g._native(g._data(data)) and g._packed
    for _ in range(20):
        g.update_sites(data)
    assert bool(torch.isfinite(g.nat1).all()) and bool(torch.isfinite(g.nat2).all()) and bool(torch.isfinite(g.log_norm).all())
    assert np.isfinite(float(g.classic_elbo(data))) and np.isfinite(float(g.energy(data)))
    assert g.num_skipped == 0
    g.dist_p.plan.check_info()
