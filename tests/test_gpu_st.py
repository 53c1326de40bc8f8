"""
GPU tests of the spatio-temporal sparse CVI model (vidp_amd.spatio_temporal_variational; kernels mfgm_st_predict_kl /
mfgm_st_site_update_q, csrc/mfgm_st.h): the two kernels against NumPy sums with a derived rounding bound, run-to-run bit equality,
null-output modes and the materialised-w twins of mfgm_sparse.h; the native routes against the torch route and the dense NumPy
model of tests/np_st.py over twenty damped steps; the known answer (exact GP regression with k_s k_t) on the device.  fp64.
"""
import ctypes

import numpy as np
import pytest

from oracle import np_kernels, np_models
from tests import np_lik, np_st

pytestmark = pytest.mark.gpu

EPS = 2.3e-16          # a little above the unit roundoff of fp64 (1.1e-16) per operation, as the issue of this feature sets it


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
    i, j = np.tril_indices(d)
    return np.concatenate([nat2[:, i, j], nat2[:, d:, :d].reshape(len(nat2), -1), nat2[:, d + i, d + j]], axis=1)


def _case(rng, Ms, dt, M1=160):
    """Random well-conditioned pair marginals given as chain blocks (built as tests/test_gpu_spep._case builds them), per-interval
    counts drawn from {0, 1, 2, 7, 300} (each value present), random a, h, c, gradients, sites and prior blocks."""
    d = Ms * dt
    n, M = 2 * d, M1 - 1
    A = rng.normal(size=(M1, n, n)) / np.sqrt(n)
    S = A @ A.transpose(0, 2, 1) + 0.5 * np.eye(n)
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
    cnt = rng.choice([0, 1, 2, 7, 300], size=M1, p=[0.3, 0.25, 0.2, 0.15, 0.1])
    cnt[:6] = (300, 0, 1, 7, 2, 300)
    cnt[-2:] = (0, 7)
    seg = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    N = int(cnt.sum())
    a = rng.normal(size=(N, Ms)) * (0.8 / np.sqrt(Ms))
    h = rng.normal(size=(N, 2 * dt)) * (0.8 / np.sqrt(2 * dt))
    return dict(Ms=Ms, dt=dt, d=d, M=M, seg=seg, cnt=cnt, idx=np.repeat(np.arange(M1), cnt), a=a, h=h, w=np_st.kron_w(a, h),
                c=rng.uniform(0.0, 0.2, size=N), g1=rng.normal(size=N), g2=-rng.uniform(0.1, 1.0, size=N), Sig=Sig, Sub=Sub, mu=mu,
                P0=P0, pm=pm, pair=pair, pmu=pmu, nat1=0.3 * rng.normal(size=(M1, n)),
                nat2=(lambda B: -0.5 * (B + B.transpose(0, 2, 1)))(rng.normal(size=(M1, n, n))),
                Pd=rng.normal(size=(M, d, d)), Ps=rng.normal(size=(M, d, d)), mup=rng.normal(size=(M, d)))


def _structs(amd, cs):
    """(mfgm_st_data, mfgm_sparse_data with the materialised w, the device tensors that back them)."""
    keep = dict(seg=dev(cs["seg"], np.int32), a=dev(cs["a"]), h=dev(cs["h"]), c=dev(cs["c"]), w=dev(cs["w"]), pm=dev(cs["pm"]),
                P0=dev(cs["P0"]))
    st = amd._lib.StData()
    st.M, st.Ms, st.dt, st.N = cs["M"], cs["Ms"], cs["dt"], len(cs["c"])
    st.seg, st.a, st.h, st.c = (keep[k].data_ptr() for k in ("seg", "a", "h", "c"))
    st.prior_mean, st.prior_cov = keep["pm"].data_ptr(), keep["P0"].data_ptr()
    sd = amd._lib.SparseData()
    sd.M, sd.d, sd.N, sd.m_lo, sd.m_hi = cs["M"], cs["d"], len(cs["c"]), 0, 0
    sd.seg, sd.w, sd.c = keep["seg"].data_ptr(), keep["w"].data_ptr(), keep["c"].data_ptr()
    sd.prior_mean, sd.prior_cov = keep["pm"].data_ptr(), keep["P0"].data_ptr()
    return st, sd, keep


def _predict(amd, cs, which, kl=True, plan=None, want_trace=True):
    """(fmu, fvar, trace, maha) on the host from mfgm_st_predict_kl (which = "st") or mfgm_sparse_predict_kl ("sparse")."""
    import torch
    from vidp_amd.packed import _ptr, _stream
    st, sd, keep = _structs(amd, cs)
    lib = amd._lib.load()
    N = len(cs["c"])
    b = [dev(cs["mu"]), dev(cs["Sig"]), dev(cs["Sub"]), dev(cs["Pd"]), dev(cs["Ps"]), dev(cs["mup"])]
    out = torch.full((2, N), 7.0, dtype=torch.float64, device="cuda")
    kt = torch.full((2,), 7.0, dtype=torch.float64, device="cuda")
    fn, data = (lib.mfgm_st_predict_kl, st) if which == "st" else (lib.mfgm_sparse_predict_kl, sd)
    amd._lib.check(fn(ctypes.byref(data), _ptr(b[0]), _ptr(b[1]), _ptr(b[2]), _ptr(out[0]), _ptr(out[1]), plan.h if kl else None, _ptr(b[3]),
                      _ptr(b[4]), -2.0, -1.0, _ptr(b[5]), _ptr(kt[0:1]) if want_trace else None, _ptr(kt[1:2]), _ptr(plan.ws), _stream()),
                   "predict_kl")
    torch.cuda.synchronize()
    return host(out[0]), host(out[1]), float(kt[0]), float(kt[1])


def _update(amd, cs, which, lr=0.7):
    from vidp_amd.packed import _ptr, _stream
    import torch
    st, sd, keep = _structs(amd, cs)
    lib = amd._lib.load()
    b = [dev(cs["g1"]), dev(cs["g2"]), dev(cs["nat1"]), dev(_pack(cs["nat2"], cs["d"]))]
    fn, data = (lib.mfgm_st_site_update_q, st) if which == "st" else (lib.mfgm_sparse_site_update_q, sd)
    amd._lib.check(fn(ctypes.byref(data), _ptr(b[0]), _ptr(b[1]), lr, _ptr(b[2]), _ptr(b[3]), _stream()), "site_update_q")
    torch.cuda.synchronize()
    return host(b[2]), host(b[3])


def _np_predict(cs):
    """(fmu, fvar, trace, maha) and the sums of absolute terms of each, from the same inputs."""
    w, idx, d = cs["w"], cs["idx"], cs["d"]
    fmu = (w * cs["pmu"][idx]).sum(-1)
    smu = (np.abs(w) * np.abs(cs["pmu"][idx])).sum(-1)
    fvar, svar = cs["c"].copy(), np.abs(cs["c"])
    for k in np.unique(idx):
        sel = idx == k
        fvar[sel] += np.einsum("ni,ij,nj->n", w[sel], cs["pair"][k], w[sel])
        svar[sel] += np.einsum("ni,ij,nj->n", np.abs(w[sel]), np.abs(cs["pair"][k]), np.abs(w[sel]))
    dv = cs["mup"] - cs["mu"]
    tr_t = [-2.0 * cs["Pd"] * cs["Sig"], 2.0 * -1.0 * cs["Ps"][:-1] * cs["Sub"][:-1]]
    mh_t = [-2.0 * cs["Pd"] * dv[:, :, None] * dv[:, None, :], 2.0 * -1.0 * cs["Ps"][:-1] * dv[1:, :, None] * dv[:-1, None, :]]
    return (fmu, fvar, sum(t.sum() for t in tr_t), sum(t.sum() for t in mh_t),
            smu, svar, sum(np.abs(t).sum() for t in tr_t), sum(np.abs(t).sum() for t in mh_t))


def _np_update(cs, lr=0.7):
    w, idx, n = cs["w"], cs["idx"], 2 * cs["d"]
    s1, a1 = np.zeros_like(cs["nat1"]), np.zeros_like(cs["nat1"])
    np.add.at(s1, idx, cs["g1"][:, None] * w)
    np.add.at(a1, idx, np.abs(cs["g1"][:, None] * w))
    s2, a2 = np.zeros_like(cs["nat2"]), np.zeros_like(cs["nat2"])
    for k in np.unique(idx):
        sel = idx == k
        s2[k] = np.einsum("n,ni,nj->ij", cs["g2"][sel], w[sel], w[sel])
        a2[k] = np.einsum("n,ni,nj->ij", np.abs(cs["g2"][sel]), np.abs(w[sel]), np.abs(w[sel]))
    d = cs["d"]
    return ((1 - lr) * cs["nat1"] + lr * s1, _pack((1 - lr) * cs["nat2"] + lr * s2, d),
            np.abs((1 - lr) * cs["nat1"]) + lr * a1, _pack(np.abs((1 - lr) * cs["nat2"]) + lr * a2, d))


SHAPES = [(5, 2), (3, 3), (16, 1), (8, 2), (10, 3), (16, 2)]


@pytest.mark.parametrize("Ms,dt", SHAPES)
def test_predict_kernel_matches_numpy_sums(amd, rng, Ms, dt):
    """mfgm_st_predict_kl against NumPy sums.  Every output is a sum of products of the inputs, so with n terms and a handful of
    roundings per term  |got - want| <= 4 n_max EPS sum|terms|  whatever the order of summation: n = 2D for fmu, (2D)^2 + 1 for fvar,
    2 M D^2 for the two KL sums.  Also: two launches agree bit for bit; plan = NULL or a null trace gives the plain prediction and
    leaves the KL outputs alone; mfgm_sparse_predict_kl fed the materialised w agrees to the same bound."""
    cs = _case(rng, Ms, dt)
    d, M = cs["d"], cs["M"]
    plan = amd.Plan(1, M, d)
    want = _np_predict(cs)
    got = _predict(amd, cs, "st", plan=plan)
    again = _predict(amd, cs, "st", plan=plan)
    ref = _predict(amd, cs, "sparse", plan=plan)
    nmax = (2 * d, (2 * d) ** 2 + 1, 2 * M * d * d, 2 * M * d * d)
    for k, name in enumerate(("fmu", "fvar", "trace", "maha")):
        bound = 4.0 * nmax[k] * EPS * want[4 + k]
        err, err_ref = np.max(np.abs(got[k] - want[k]) / bound), np.max(np.abs(got[k] - ref[k]) / bound)
        print(f"st predict Ms={Ms} dt={dt} {name}: |got - numpy| / bound {err:.3e}, |got - materialised-w kernel| / bound {err_ref:.3e}")
        assert err <= 1.0 and err_ref <= 1.0
        assert np.array_equal(got[k], again[k])
    for kw in (dict(kl=False), dict(want_trace=False)):
        plain = _predict(amd, cs, "st", plan=plan, **kw)
        assert np.array_equal(plain[0], got[0]) and np.array_equal(plain[1], got[1]) and plain[2] == 7.0 and plain[3] == 7.0
    plan.check_info()


@pytest.mark.parametrize("Ms,dt", SHAPES)
def test_site_update_kernel_matches_numpy_sums(amd, rng, Ms, dt):
    """mfgm_st_site_update_q against NumPy sums: an entry is (1 - lr) old + lr sum_i g_i w_i[r] w_i[c] over at most 300 points, bound
    4 (n_m + 1) EPS sum|terms| with n_max = 301; two launches agree bit for bit; mfgm_sparse_site_update_q fed the materialised w
    agrees to the same bound; intervals without data decay by (1 - lr) exactly."""
    cs = _case(rng, Ms, dt)
    want = _np_update(cs)
    got, again, ref = _update(amd, cs, "st"), _update(amd, cs, "st"), _update(amd, cs, "sparse")
    for k, name in enumerate(("nat1", "nat2q")):
        bound = 4.0 * 301 * EPS * want[2 + k]
        ok = bound > 0
        err = np.max(np.abs(got[k] - want[k])[ok] / bound[ok])
        err_ref = np.max(np.abs(got[k] - ref[k])[ok] / bound[ok])
        print(f"st sites Ms={Ms} dt={dt} {name}: |got - numpy| / bound {err:.3e}, |got - materialised-w kernel| / bound {err_ref:.3e}")
        assert err <= 1.0 and err_ref <= 1.0
        assert np.array_equal(got[k][~ok], want[k][~ok])
        assert np.array_equal(got[k], again[k])
    empty = cs["cnt"] == 0
    assert empty.sum() > 10
    np.testing.assert_array_equal(got[0][empty], ((1 - 0.7) * cs["nat1"])[empty])
    np.testing.assert_array_equal(got[1][empty], _pack((1 - 0.7) * cs["nat2"], cs["d"])[empty])


def _liks(kind):
    from vidp_amd.likelihoods import Bernoulli, Gaussian, Poisson
    return {"gaussian": (lambda: Gaussian(0.6), np_models.GaussianLik(0.6)), "bernoulli": (lambda: Bernoulli(1e-3), np_lik.Bernoulli(1e-3)),
            "poisson": (lambda: Poisson(1.3), np_lik.Poisson(1.3))}[kind]


def _offgrid(rng, kind, Ms, M, N):
    gx, gy = np.meshgrid(np.linspace(-1.0, 1.0, (Ms + 1) // 2), [-0.4, 0.4], indexing="ij")
    zs = np.stack([gx.reshape(-1), gy.reshape(-1)], axis=1)[:Ms]
    zt = 0.25 * np.arange(M)
    X = np.concatenate([rng.uniform(-1.2, 1.2, size=(N, 2)), np.sort(rng.uniform(-0.3, zt[-1] + 0.3, size=N))[:, None]], axis=1)
    f = 1.2 * np.sin(0.8 * X[:, -1]) * np.cos(X[:, 0])
    if kind == "gaussian":
        y = f + np.sqrt(0.6) * rng.normal(size=N)
    elif kind == "bernoulli":
        y = (f + 0.5 * rng.normal(size=N) > 0).astype(np.float64)
    else:
        y = rng.poisson(np.exp(0.5 * f)).astype(np.float64)
    return zs, zt, X, y[:, None]


@pytest.mark.parametrize("kind", ["gaussian", "bernoulli", "poisson"])
@pytest.mark.parametrize("Ms", [8, 3])
def test_native_model_against_torch_route_and_numpy(amd, rng, monkeypatch, Ms, kind):
    """The native route follows the torch route of the same class (VIDP_FUSED_SPARSE=0) and the dense NumPy model over twenty damped
    steps (lr = 0.5) at 1e-8: Matern-3/2 in time, 400 time inducing points 0.25 lengthscales apart, 12 000 off-grid points.  Ms = 8
    (D = 16) runs the factored kernels on the packed sites, Ms = 3 (D = 6) the materialised w on dense sites."""
    from vidp_amd import kernels as K, space_kernels as SK
    from vidp_amd.spatio_temporal_variational import SpatioTemporalSparseCVI
    zs, zt, X, y = _offgrid(rng, kind, Ms, 400, 12000)
    var = 0.25 if kind == "poisson" else 1.0
    mk, olik = _liks(kind)
    new = lambda: SpatioTemporalSparseCVI(dev(zs), dev(zt), SK.Matern32([0.9, 1.2], 1.0), K.Matern32(1.0, var), mk(), learning_rate=0.5)
    data = (dev(X), dev(y))
    a = new()
    da = a._data(data)
    assert da is not None and da["factored"] == (Ms == 8) and a._packed == (Ms == 8)
    monkeypatch.setenv("VIDP_FUSED_SPARSE", "0")
    b = new()
    assert b._data(data) is None
    monkeypatch.delenv("VIDP_FUSED_SPARSE")
    o = np_st.SpatioTemporalSparseCVI(zs, zt, np_st.SpaceKernel("matern32", [0.9, 1.2], 1.0), np_kernels.Matern32(1.0, var), olik,
                                      learning_rate=0.5)
    tol = 1e-8
    for step in range(20):
        a.update_sites(data)
        monkeypatch.setenv("VIDP_FUSED_SPARSE", "0")
        b.update_sites(data)
        eb = float(b.elbo(data))
        monkeypatch.delenv("VIDP_FUSED_SPARSE")
        o.update_sites(X, y)
        for x, w1, w2 in ((a.nat1, b.nat1, o.nat1), (a.nat2, b.nat2, o.nat2)):
            np.testing.assert_allclose(host(x), host(w1), rtol=tol, atol=tol * np.abs(w2).max())
            np.testing.assert_allclose(host(x), w2, rtol=tol, atol=tol * np.abs(w2).max())
        ea, eo = float(a.elbo(data)), o.elbo(X, y)
        if step in (0, 19):
            print(f"st model Ms={Ms} {kind} step {step}: elbo native {ea!r} torch {eb!r} numpy {eo!r}")
        np.testing.assert_allclose(ea, eb, rtol=tol)
        np.testing.assert_allclose(ea, eo, rtol=tol)
    fm, fv = a.space_time_predict_f(data[0])
    om, ov = o.predict_f(X)
    np.testing.assert_allclose(host(fm), om, rtol=tol, atol=tol)
    np.testing.assert_allclose(host(fv), ov, rtol=tol, atol=tol)
    if kind != "gaussian":
        np.testing.assert_allclose(host(a.predict_log_density(data)), o.predict_log_density(X, y), rtol=tol, atol=tol)
    a.dist_p.plan.check_info()


def _time_cov(order, ls, var):
    def k(tau):
        r = np.abs(tau) / ls
        if order == 2:
            return var * (1.0 + np.sqrt(3.0) * r) * np.exp(-np.sqrt(3.0) * r)
        return var * (1.0 + np.sqrt(5.0) * r + 5.0 / 3.0 * r * r) * np.exp(-np.sqrt(5.0) * r)
    return k


def _linear_mean(X):
    import torch
    w = np.arange(1.0, X.shape[1] + 1.0)
    return (X @ (dev(w) if torch.is_tensor(X) else w))[:, None] + 3.0


@pytest.mark.parametrize("with_mean", [False, True])
@pytest.mark.parametrize("Ms,order", [(5, 2), (10, 3)])
def test_known_answer_on_the_device(amd, rng, Ms, order, with_mean):
    """Data on the grid Z_s x Z_t (40 times 0.25 lengthscales apart, Z_s 0.5 lengthscales apart), Gaussian likelihood, learning_rate 1,
    ten update_sites on the factored route: elbo and space_time_predict_f equal dense GP regression with k_s k_t at the reference's
    atol = rtol = 1e-6.  D = 10 (Ms = 5, Matern-3/2) and D = 30 (Ms = 10, Matern-5/2)."""
    from vidp_amd import kernels as K, space_kernels as SK
    from vidp_amd.likelihoods import Gaussian
    from vidp_amd.spatio_temporal_variational import SpatioTemporalSparseCVI
    zs, zt = 0.5 * np.arange(float(Ms))[:, None], 0.25 * np.arange(40.0)
    X = np.concatenate([np.repeat(zs[None], len(zt), 0), np.repeat(zt[:, None, None], Ms, 1)], axis=-1).reshape(-1, 2)
    mean = _linear_mean if with_mean else None
    Y = rng.normal(size=(X.shape[0], 1)) + (0.0 if mean is None else mean(X))
    kt = K.Matern32(1.0, 1.0) if order == 2 else K.Matern52(1.0, 1.0)
    m = SpatioTemporalSparseCVI(dev(zs), dev(zt), SK.Matern32(1.0, 1.0), kt, Gaussian(1.0), mean_function=mean, learning_rate=1.0)
    data = (dev(X), dev(Y))
    assert m._data(data)["factored"] and m.kernel.state_dim == Ms * (order if order == 2 else 3)
    for _ in range(10):
        m.update_sites(data)
    lml, post_mean = np_st.gpr(np_st.SpaceKernel("matern32", 1.0, 1.0), _time_cov(order, 1.0, 1.0), X, Y, 1.0, mean)
    got = float(m.elbo(data))
    print(f"known answer on the device D={m.kernel.state_dim} mean={with_mean}: elbo {got!r} log marginal likelihood {lml!r}")
    assert np.allclose(got, lml, atol=1e-6, rtol=1e-6)
    assert np.allclose(host(m.space_time_predict_f(data[0])[0])[:, 0], post_mean, atol=1e-6, rtol=1e-6)
    m.dist_p.plan.check_info()


@pytest.mark.parametrize("Ms,kind", [(3, "gaussian"), (3, "poisson"), (5, "gaussian"), (5, "bernoulli")])
def test_mean_function_on_the_device_routes(amd, rng, monkeypatch, Ms, kind):
    """A linear mean function on both device routes (Ms = 3: D = 6, materialised w on dense sites; Ms = 5: D = 10, factored kernels)
    against the torch route and the dense NumPy model over ten damped steps at 1e-8; then space_time_predict_f at new inputs, sorted
    (the kernels of update_sites) and shuffled (the torch route), against the NumPy model."""
    from vidp_amd import kernels as K, space_kernels as SK
    from vidp_amd.spatio_temporal_variational import SpatioTemporalSparseCVI
    zs, zt, X, y = _offgrid(rng, kind, Ms, 60, 1500)
    # a small slope keeps the Poisson rates moderate; smaller still for Bernoulli, whose jittered probit is not log-concave in the
    # tails: with |mean| > 2 a mislabelled point gets a positive site precision and the dense NumPy posterior stops being positive definite
    scale = {"gaussian": 1.0, "poisson": 0.05, "bernoulli": 0.01}[kind]
    mean = lambda Z: scale * _linear_mean(Z)
    if kind == "gaussian":
        y = y + mean(X)
    var = 0.25 if kind == "poisson" else 1.0
    mk, olik = _liks(kind)
    new = lambda: SpatioTemporalSparseCVI(dev(zs), dev(zt), SK.Matern32([0.9, 1.2], 1.0), K.Matern32(1.0, var), mk(), mean_function=mean,
                                          learning_rate=0.5)
    data = (dev(X), dev(y))
    a = new()
    assert a._data(data)["factored"] == (Ms == 5) and a._data(data)["mean"] is not None
    monkeypatch.setenv("VIDP_FUSED_SPARSE", "0")
    b = new()
    assert b._data(data) is None
    monkeypatch.delenv("VIDP_FUSED_SPARSE")
    o = np_st.SpatioTemporalSparseCVI(zs, zt, np_st.SpaceKernel("matern32", [0.9, 1.2], 1.0), np_kernels.Matern32(1.0, var), olik,
                                      mean_function=mean, learning_rate=0.5)
    tol = 1e-8
    for _ in range(10):
        a.update_sites(data)
        monkeypatch.setenv("VIDP_FUSED_SPARSE", "0")
        b.update_sites(data)
        eb = float(b.elbo(data))
        monkeypatch.delenv("VIDP_FUSED_SPARSE")
        o.update_sites(X, y)
        for x, w1, w2 in ((a.nat1, b.nat1, o.nat1), (a.nat2, b.nat2, o.nat2)):
            np.testing.assert_allclose(host(x), host(w1), rtol=tol, atol=tol * np.abs(w2).max())
            np.testing.assert_allclose(host(x), w2, rtol=tol, atol=tol * np.abs(w2).max())
        np.testing.assert_allclose(float(a.elbo(data)), eb, rtol=tol)
        np.testing.assert_allclose(float(a.elbo(data)), o.elbo(X, y), rtol=tol)
    _, _, Xn, _ = _offgrid(rng, kind, Ms, 60, 700)
    for Z in (Xn, Xn[rng.permutation(len(Xn))], X):
        Zd = dev(Z)
        sorted_dev = a._build_data(Zd) is not None
        assert sorted_dev == bool(np.all(np.diff(Z[:, -1]) >= 0))
        fm, fv = a.space_time_predict_f(Zd)
        om, ov = o.predict_f(Z)
        np.testing.assert_allclose(host(fm), om, rtol=tol, atol=tol)
        np.testing.assert_allclose(host(fv), ov, rtol=tol, atol=tol)
    # predicting elsewhere leaves the training data's cached predictions in place
    assert a._pred_cache[1] is a._data(data)
    a.dist_p.plan.check_info()


@pytest.mark.parametrize("Ms", [3, 8])
def test_chain_objects_on_the_device(amd, rng, Ms):
    """dist_p, dist_q and posterior of the model on the device: dist_q's marginals are the model's cached ones; posterior.predict_f
    gives the moments of u(t) = f(Z_s, t), from which the reference's space_time_predict_f (batch_base_conditional, :149-183)
        a = chol(K_zz)^-1 k_s(Z_s, x),  A2 = chol(K_zz)^-T a,  mean = A2^T E[u],  var = k_s(x, x) - |a|^2 + A2^T Cov[u] A2
    reproduces the model's space_time_predict_f."""
    import torch
    from vidp_amd import kernels as K, space_kernels as SK
    from vidp_amd.spatio_temporal_variational import SpatioTemporalSparseCVI
    zs, zt, X, y = _offgrid(rng, "bernoulli", Ms, 50, 900)
    mk, _ = _liks("bernoulli")
    ks = SK.Matern32([0.9, 1.2], 1.0)
    m = SpatioTemporalSparseCVI(dev(zs), dev(zt), ks, K.Matern32(1.0, 1.0), mk(), learning_rate=0.5)
    data = (dev(X), dev(y))
    for _ in range(5):
        m.update_sites(data)
    D = m.kernel.state_dim
    p, q = m.dist_p, m.dist_q
    pm, pc = p.marginals
    assert tuple(pm.shape[-2:]) == (50, D) and float(pm.abs().max()) == 0.0
    np.testing.assert_allclose(host(pc.reshape(50, D, D)[7]), host(m.kernel.initial_covariance_matrix()), rtol=1e-9, atol=1e-12)
    qm, qc = q.marginals
    mg = m._marginals()
    np.testing.assert_allclose(host(qm.reshape(50, D)), host(mg["mu"]), rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(host(qc.reshape(50, D, D)), host(mg["Sig"]), rtol=1e-8, atol=1e-10)
    mean_u, cov_u = m.posterior.predict_f(data[0][:, -1].contiguous(), full_output_cov=True)
    assert tuple(mean_u.shape) == (900, Ms) and tuple(cov_u.shape) == (900, Ms, Ms)
    L = torch.linalg.cholesky(ks.K(dev(zs)))
    a = torch.linalg.solve_triangular(L, ks.K(dev(zs), data[0][:, :-1]), upper=False)
    A2 = torch.linalg.solve_triangular(L.T, a, upper=True).T                    # [N, Ms]
    want_m = (A2 * mean_u).sum(-1)
    want_v = 1.0 - (a * a).sum(0) + torch.einsum("ni,nij,nj->n", A2, cov_u, A2)
    fm, fv = m.space_time_predict_f(data[0])
    np.testing.assert_allclose(host(fm)[:, 0], host(want_m), rtol=1e-8, atol=1e-9)
    np.testing.assert_allclose(host(fv)[:, 0], host(want_v), rtol=1e-8, atol=1e-9)
    p.plan.check_info()


def test_materialised_w_route_equals_the_factored_one(amd, rng, monkeypatch):
    """VIDP_ST_FACTORED=0 (D = 16: w [N, 2D] through mfgm_sparse_predict_kl / mfgm_sparse_site_update_q, the yardstick of
    tools/st_rate.py) follows the factored route over ten damped steps: the same sums in another order, 1e-11 of the largest site."""
    from vidp_amd import kernels as K, space_kernels as SK
    from vidp_amd.spatio_temporal_variational import SpatioTemporalSparseCVI
    zs, zt, X, y = _offgrid(rng, "bernoulli", 8, 100, 4000)
    mk, _ = _liks("bernoulli")
    new = lambda: SpatioTemporalSparseCVI(dev(zs), dev(zt), SK.Matern32([0.9, 1.2], 1.0), K.Matern32(1.0, 1.0), mk(), learning_rate=0.5)
    data = (dev(X), dev(y))
    a, b = new(), new()
    assert a._data(data)["factored"]
    monkeypatch.setenv("VIDP_ST_FACTORED", "0")          # read when a data set's constants are built
    assert not b._data(data)["factored"] and b._packed
    monkeypatch.delenv("VIDP_ST_FACTORED")
    for _ in range(10):
        a.update_sites(data)
        b.update_sites(data)
        for x, w in ((a.nat1, b.nat1), (a._nat2q, b._nat2q)):
            np.testing.assert_allclose(host(x), host(w), rtol=1e-9, atol=1e-11 * float(w.abs().max()))
        np.testing.assert_allclose(float(a.elbo(data)), float(b.elbo(data)), rtol=1e-11)
