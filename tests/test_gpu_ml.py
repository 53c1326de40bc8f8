"""
GPU tests of the multi-latent sparse CVI model (vidp_amd.multi_latent_variational; kernels mfgm_ml_predict_lik / mfgm_ml_site_update /
mfgm_ml_site_update_q, csrc/mfgm_ml.h): the kernels against NumPy sums with a derived rounding bound, run-to-run bit equality,
null-output modes, the coupled likelihoods at the device's own marginals, the site update against mfgm_sparse_site_update[_q] called
once per latent; the native route against the torch route and the dense NumPy model of tests/np_ml.py over twenty damped steps; the
decomposition of MultiStage into three scalar SparseCVIGaussianProcess models on the device; graph capture of the step.  fp64.
"""
import ctypes

import numpy as np
import pytest

from oracle import np_kernels
from tests import np_ml

pytestmark = pytest.mark.gpu

EPS = 2.3e-16          # a little above the unit roundoff of fp64 per operation, as in tests/test_gpu_st.py


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


DLS = [(1, 1), (2, 1, 3), (2, 2, 2), (3, 3, 3), (8, 8), (16, 16), (1,) * 8, (4,) * 8, (16, 1)]
_ids = lambda dl: "x".join(str(n) for n in dl)


def _case(rng, dl, M1=160):
    """Random well-conditioned pair marginals given as chain blocks (built as tests/test_gpu_st._case builds them: FULL pair
    covariances, cross-latent blocks included), per-interval counts drawn from {0, 1, 2, 7, 300} (each value present), random rows
    h [N, 2D], c [N, L], gradients [N, L], observations, sites and prior blocks."""
    d, L = sum(dl), len(dl)
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
    h = rng.normal(size=(N, n)) * (0.8 / np.sqrt(2 * max(dl)))
    y3 = rng.choice([0.0, 1.0, 2.0, 3.0, 9.0, -1.0, 0.5, 1.5, np.nan], size=N, p=[0.25, 0.2, 0.15, 0.15, 0.05, 0.05, 0.05, 0.05, 0.05])
    return dict(dl=dl, L=L, d=d, M=M, seg=seg, cnt=cnt, idx=np.repeat(np.arange(M1), cnt), h=h, c=rng.uniform(0.0, 0.2, size=(N, L)),
                g1=rng.normal(size=(N, L)), g2=-rng.uniform(0.1, 1.0, size=(N, L)), y3=y3, y2=rng.normal(size=N) * 1.5, Sig=Sig, Sub=Sub,
                mu=mu, P0=P0, pm=pm, pair=pair, pmu=pmu, nat1=0.3 * rng.normal(size=(M1, n)),
                nat2=(lambda B: -0.5 * (B + B.transpose(0, 2, 1)))(rng.normal(size=(M1, n, n))))


def _struct(amd, cs):
    keep = dict(seg=dev(cs["seg"], np.int32), h=dev(cs["h"]), c=dev(cs["c"]), pm=dev(cs["pm"]), P0=dev(cs["P0"]))
    s = amd._lib.MlData()
    s.M, s.L, s.N = cs["M"], cs["L"], len(cs["h"])
    for k, n in enumerate(cs["dl"]):
        s.dl[k] = n
    s.seg, s.h, s.c = (keep[k].data_ptr() for k in ("seg", "h", "c"))
    s.prior_mean, s.prior_cov = keep["pm"].data_ptr(), keep["P0"].data_ptr()
    return s, keep


def _lik(amd, kind):
    q = amd._lib.MlLik()
    q.kind, q.param[0], q.param[1] = kind, 2e-3, 1.3
    return q


def _predict(amd, cs, kind, want=("fmu", "fvar", "ve", "g1", "g2")):
    """The five outputs on the host; buffers of outputs not asked for are passed as NULL and keep their sentinel 7."""
    import torch
    from vidp_amd.packed import _ptr, _stream
    s, keep = _struct(amd, cs)
    q = _lik(amd, kind)
    N, L = len(cs["h"]), cs["L"]
    b = [dev(cs["mu"]), dev(cs["Sig"]), dev(cs["Sub"])]
    y = None if kind == 0 else dev(cs["y3"] if kind == 1 else cs["y2"])
    out = {k: torch.full((N, L), 7.0, dtype=torch.float64, device="cuda") for k in ("fmu", "fvar", "g1", "g2")}
    out["ve"] = torch.full((cs["M"] + 1,), 7.0, dtype=torch.float64, device="cuda")
    p = lambda k: _ptr(out[k]) if k in want else None
    amd._lib.check(amd._lib.load().mfgm_ml_predict_lik(ctypes.byref(s), ctypes.byref(q), _ptr(y), _ptr(b[0]), _ptr(b[1]), _ptr(b[2]), p("fmu"),
                                                       p("fvar"), p("ve"), p("g1"), p("g2"), _stream()), "mfgm_ml_predict_lik")
    torch.cuda.synchronize()
    return {k: host(v) for k, v in out.items()}


@pytest.mark.parametrize("dl", DLS, ids=_ids)
def test_predict_kernel_matches_numpy_sums(amd, rng, dl):
    """mfgm_ml_predict_lik with MFGM_ML_NONE against NumPy sums: every output is a sum of products of the inputs, so with n terms
    |got - want| <= 4 n EPS sum|terms| whatever the order of summation, n = 2 max dl for fmu and (2 max dl)^2 + 1 for fvar.  The pair
    covariances are full (cross-latent blocks included): only the within-latent blocks may be read.  Two launches agree bit for bit;
    a NULL output is not written."""
    cs = _case(rng, dl)
    fmu, fvar, smu, svar = np_ml.predict_sums(cs["h"], cs["c"], cs["idx"], cs["pmu"], cs["pair"], dl)
    got = _predict(amd, cs, 0, want=("fmu", "fvar"))
    again = _predict(amd, cs, 0, want=("fmu", "fvar"))
    nd = 2 * max(dl)
    for name, g, w, sc, n in (("fmu", got["fmu"], fmu, smu, nd), ("fvar", got["fvar"], fvar, svar, nd * nd + 1)):
        err = np.max(np.abs(g - w) / (4.0 * n * EPS * sc))
        print(f"ml predict dl={dl} {name}: |got - numpy| / bound {err:.3e}")
        assert err <= 1.0
        assert np.array_equal(g, again[name])
    for k in ("ve", "g1", "g2"):
        assert np.all(got[k] == 7.0)
    only = _predict(amd, cs, 0, want=("fvar",))
    assert np.array_equal(only["fvar"], got["fvar"]) and np.all(only["fmu"] == 7.0)
    only = _predict(amd, cs, 0, want=("fmu",))
    assert np.array_equal(only["fmu"], got["fmu"]) and np.all(only["fvar"] == 7.0)


@pytest.mark.parametrize("dl", [dl for dl in DLS if len(dl) in (2, 3)], ids=_ids)
def test_predict_kernel_likelihood(amd, rng, dl):
    """Kinds 1 (L = 3) and 2 (L = 2): g1, g2 and the per-point VE (ve_part of the intervals with one point) against tests/np_ml.py
    evaluated at the device's own fmu, fvar, within 1e-12 of the sum of absolute terms (the bound of tests/test_gpu_lik.py); ve_part
    within (1e-12 + 4 301 EPS) sum|terms|; empty intervals give 0; two launches agree bit for bit; NULL outputs are not written and
    the others do not change."""
    cs = _case(rng, dl)
    kind = 1 if len(dl) == 3 else 2
    olik, y = (np_ml.MultiStage(2e-3, 1.3), cs["y3"]) if kind == 1 else (np_ml.HetGauss(), cs["y2"])
    got, again = _predict(amd, cs, kind), _predict(amd, cs, kind)
    plain = _predict(amd, cs, 0, want=("fmu", "fvar"))
    assert np.array_equal(got["fmu"], plain["fmu"]) and np.array_equal(got["fvar"], plain["fvar"])
    ve, g1, g2, sc = np_ml.grads_expectation(olik, got["fmu"], got["fvar"], y)
    for name, g, w, s in (("g1", got["g1"], g1, sc["g1"]), ("g2", got["g2"], g2, sc["g2"])):
        ok = s > 0
        err = np.max(np.abs(g - w)[ok] / (1e-12 * s[ok]))
        print(f"ml lik dl={dl} kind={kind} {name}: |got - numpy| / (1e-12 sum|terms|) {err:.3e}")
        assert err <= 1.0
        assert np.array_equal(g[~ok], w[~ok])
    if kind == 1:
        with np.errstate(invalid="ignore"):
            nothing = ~((y == 0) | (y == 1) | (y >= 2))
        assert nothing.sum() > 50 and np.all(got["g1"][nothing] == 0.0) and np.all(got["g2"][nothing] == 0.0)
    part = np.zeros(cs["M"] + 1)
    spart = np.zeros(cs["M"] + 1)
    np.add.at(part, cs["idx"], ve)
    np.add.at(spart, cs["idx"], sc["ve"])
    single = cs["cnt"] == 1
    at = cs["seg"][:-1][single]
    ok = sc["ve"][at] > 0
    err1 = np.max(np.abs(got["ve"][single] - ve[at])[ok] / (1e-12 * sc["ve"][at][ok]))
    okp = spart > 0
    errp = np.max(np.abs(got["ve"] - part)[okp] / ((1e-12 + 4.0 * 301 * EPS) * spart[okp]))
    print(f"ml lik dl={dl} kind={kind}: per-point VE / bound {err1:.3e}, ve_part / bound {errp:.3e}")
    assert err1 <= 1.0 and errp <= 1.0
    assert np.all(got["ve"][~okp] == 0.0) and np.all(got["ve"][cs["cnt"] == 0] == 0.0)
    for k in got:
        assert np.array_equal(got[k], again[k], equal_nan=True)
    some = _predict(amd, cs, kind, want=("g2", "ve"))
    assert np.array_equal(some["g2"], got["g2"]) and np.array_equal(some["ve"], got["ve"])
    assert all(np.all(some[k] == 7.0) for k in ("fmu", "fvar", "g1"))


def _update(amd, cs, packed, lr=0.7):
    import torch
    from vidp_amd.packed import _ptr, _stream
    s, keep = _struct(amd, cs)
    lib = amd._lib.load()
    b = [dev(cs["g1"]), dev(cs["g2"]), dev(cs["nat1"]), dev(_pack(cs["nat2"], cs["d"]) if packed else cs["nat2"])]
    fn = lib.mfgm_ml_site_update_q if packed else lib.mfgm_ml_site_update
    amd._lib.check(fn(ctypes.byref(s), _ptr(b[0]), _ptr(b[1]), lr, _ptr(b[2]), _ptr(b[3]), _stream()), "mfgm_ml_site_update")
    torch.cuda.synchronize()
    return host(b[2]), host(b[3])


def _update_per_latent(amd, cs, packed, lr=0.7):
    """mfgm_sparse_site_update[_q] once per latent with the masked row w_l = h * slots_l and that latent's gradients: latent 0 on
    the old sites (which takes the decay), the others on zero sites; the results are added on the host."""
    import torch
    from vidp_amd.packed import _ptr, _stream
    lib = amd._lib.load()
    mask = np_ml.slots(cs["dl"])
    seg, c0, pm, P0 = dev(cs["seg"], np.int32), dev(cs["c"][:, 0]), dev(cs["pm"]), dev(cs["P0"])
    fn = lib.mfgm_sparse_site_update_q if packed else lib.mfgm_sparse_site_update
    tot1, tot2 = 0.0, 0.0
    for l in range(cs["L"]):
        w = dev(cs["h"] * mask[l])
        sd = amd._lib.SparseData()
        sd.M, sd.d, sd.N, sd.m_lo, sd.m_hi = cs["M"], cs["d"], len(cs["h"]), 0, 0
        sd.seg, sd.w, sd.c, sd.prior_mean, sd.prior_cov = seg.data_ptr(), w.data_ptr(), c0.data_ptr(), pm.data_ptr(), P0.data_ptr()
        n1 = cs["nat1"] if l == 0 else np.zeros_like(cs["nat1"])
        n2 = cs["nat2"] if l == 0 else np.zeros_like(cs["nat2"])
        b = [dev(cs["g1"][:, l]), dev(cs["g2"][:, l]), dev(n1), dev(_pack(n2, cs["d"]) if packed else n2)]
        amd._lib.check(fn(ctypes.byref(sd), _ptr(b[0]), _ptr(b[1]), lr, _ptr(b[2]), _ptr(b[3]), _stream()), "mfgm_sparse_site_update")
        torch.cuda.synchronize()
        tot1, tot2 = tot1 + host(b[2]), tot2 + host(b[3])
    return tot1, tot2


@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
@pytest.mark.parametrize("dl", DLS, ids=_ids)
def test_site_update_kernel_matches_numpy_sums(amd, rng, dl, packed):
    """mfgm_ml_site_update / _q against NumPy sums: an entry is (1 - lr) old + lr sum_i g_i h_i[r] h_i[c] over at most 300 points,
    bound 4 301 EPS sum|terms|; entries whose bound is 0 are equal exactly; cross-latent entries and empty intervals equal
    (1 - lr) old exactly; the dense form is symmetric to the bit; two launches agree bit for bit; mfgm_sparse_site_update[_q] called
    once per latent with the masked row and composed on the host agrees to the same bound."""
    cs = _case(rng, dl)
    lr, d = 0.7, cs["d"]
    w1, w2, a1, a2 = np_ml.site_sums(cs["h"], cs["idx"], cs["g1"], cs["g2"], cs["nat1"], cs["nat2"], dl, lr)
    mask = np_ml.slots(dl)
    cross = np.broadcast_to((mask.T @ mask) == 0, cs["nat2"].shape)
    decay = (1 - lr) * cs["nat2"]
    if packed:
        w2, a2, cross, decay = _pack(w2, d), _pack(a2, d), _pack(cross, d), _pack(decay, d)
    got, again, ref = _update(amd, cs, packed), _update(amd, cs, packed), _update_per_latent(amd, cs, packed)
    for k, (name, want, sc) in enumerate((("nat1", w1, a1), ("nat2", w2, a2))):
        bound = 4.0 * 301 * EPS * sc
        ok = bound > 0
        err = np.max(np.abs(got[k] - want)[ok] / bound[ok])
        err_ref = np.max(np.abs(got[k] - ref[k])[ok] / bound[ok])
        print(f"ml sites dl={dl} packed={packed} {name}: |got - numpy| / bound {err:.3e}, |got - per-latent scalar kernel| / bound {err_ref:.3e}")
        assert err <= 1.0 and err_ref <= 1.0
        assert np.array_equal(got[k][~ok], want[~ok])
        assert np.array_equal(got[k], again[k])
    if len(dl) > 1:
        assert cross.sum() > 0
    assert np.array_equal(got[1][cross], decay[cross])
    empty = cs["cnt"] == 0
    assert empty.sum() > 10
    np.testing.assert_array_equal(got[0][empty], ((1 - lr) * cs["nat1"])[empty])
    np.testing.assert_array_equal(got[1][empty], decay[empty])
    if not packed:
        assert np.array_equal(got[1], got[1].transpose(0, 2, 1))


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def _setup(name):
    """(torch child kernels, oracle child kernels, likelihood maker, oracle likelihood, data maker) of a model case.  The inducing
    points lie 0.25 apart and no lengthscale exceeds 1: 0.25 lengthscales apart for the longest one.  (On longer lengthscales the
    prior precision of the Matern-5/2 components is so ill-conditioned on this grid that the torch route, the native route and the dense
    NumPy model -- three orders of summation -- differ by more than 1e-8 from one another.)"""
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import HeteroskedasticGaussian, MultiStageLikelihood
    ms = (lambda: MultiStageLikelihood(1e-3, 1.3), np_ml.MultiStage(1e-3, 1.3), np_ml.multistage_data)
    hg = (HeteroskedasticGaussian, np_ml.HetGauss(), np_ml.hetgauss_data)
    if name == "multistage5":
        kids = lambda m: [m.Matern32(1.0, 1.0), m.Matern32(0.8, 0.8), m.Matern12(1.0, 0.25)]
        return (kids(K), kids(np_kernels)) + ms
    if name == "multistage9":
        kids = lambda m: [m.Matern52(1.0, 1.0), m.Matern52(0.8, 0.8), m.Matern52(0.9, 0.25)]
        return (kids(K), kids(np_kernels)) + ms
    if name == "hetgauss5":
        kids = lambda m: [m.Matern52(1.0, 1.0), m.Matern32(0.8, 0.5)]
        return (kids(K), kids(np_kernels)) + hg
    kids = lambda m: [m.Sum([m.Matern52(1.0, 0.6), m.Matern52(0.7, 0.3), m.Matern32(0.8, 0.1)]),
                      m.Sum([m.Matern52(1.0, 0.3), m.Matern52(0.6, 0.1), m.Matern32(0.9, 0.1)])]
    return (kids(K), kids(np_kernels)) + hg


@pytest.mark.parametrize("name", ["multistage5", "multistage9", "hetgauss5", "hetgauss16"])
def test_native_model_against_torch_route_and_numpy(amd, rng, monkeypatch, name):
    """The native route follows the torch route of the same class (VIDP_NATIVE_ML=0) and the dense NumPy model over twenty damped
    steps (lr = 0.5) at 1e-8: 400 inducing points 0.25 lengthscales apart, 12 000 points.  D = 5: dense sites; D = 9, 16: packed
    sites.  Then predict_f at new times (sorted: the kernel; shuffled: the torch route) and posterior.predict_f against NumPy."""
    from vidp_amd import kernels as K
    from vidp_amd.multi_latent_variational import MultiLatentSparseCVI
    kids, okids, mk, olik, make = _setup(name)
    z = 0.25 * np.arange(400.0)
    t, y = make(rng, z, 12000)
    new = lambda: MultiLatentSparseCVI(K.IndependentMultiOutput(kids), dev(z), mk(), learning_rate=0.5)
    data = (dev(t), dev(y))
    a = new()
    D = a.kernel.state_dim
    assert D == {"multistage5": 5, "multistage9": 9, "hetgauss5": 5, "hetgauss16": 16}[name]
    assert a._data(data) is not None and a._packed == (D > 8)
    monkeypatch.setenv("VIDP_NATIVE_ML", "0")
    b = new()
    assert b._data(data) is None
    monkeypatch.delenv("VIDP_NATIVE_ML")
    o = np_ml.MultiLatentSparseCVI(okids, z, olik, learning_rate=0.5)
    tol = 1e-8
    for step in range(20):
        a.update_sites(data)
        monkeypatch.setenv("VIDP_NATIVE_ML", "0")
        b.update_sites(data)
        eb = float(b.elbo(data))
        monkeypatch.delenv("VIDP_NATIVE_ML")
        o.update_sites(t, y)
        for x, w1, w2 in ((a.nat1, b.nat1, o.nat1), (a.nat2, b.nat2, o.nat2)):
            np.testing.assert_allclose(host(x), host(w1), rtol=tol, atol=tol * np.abs(w2).max())
            np.testing.assert_allclose(host(x), w2, rtol=tol, atol=tol * np.abs(w2).max())
        ea, eo = float(a.elbo(data)), o.elbo(t, y)
        if step in (0, 19):
            print(f"ml model {name} step {step}: elbo native {ea!r} torch {eb!r} numpy {eo!r}")
        np.testing.assert_allclose(ea, eb, rtol=tol)
        np.testing.assert_allclose(ea, eo, rtol=tol)
    tn = np.sort(rng.uniform(z[0] - 0.5, z[-1] + 0.5, size=700))
    for tt in (tn, tn[rng.permutation(len(tn))]):
        om, ov = o.predict_f(tt)
        for fm, fv in (a.predict_f(dev(tt)), a.posterior.predict_f(dev(tt))):
            assert tuple(fm.shape) == (700, len(kids))
            np.testing.assert_allclose(host(fm), om, rtol=tol, atol=tol)
            np.testing.assert_allclose(host(fv), ov, rtol=tol, atol=tol)
    fm, fv = a.predict_f_at_data(data)
    om, ov = o.predict_f(t)
    np.testing.assert_allclose(host(fm), om, rtol=tol, atol=tol)
    np.testing.assert_allclose(host(fv), ov, rtol=tol, atol=tol)
    with pytest.raises(NotImplementedError):
        a.predict_log_density(data)
    a.dist_p.plan.check_info()


@pytest.mark.parametrize("name", ["multistage5", "multistage9"])
def test_multistage_decomposes_on_the_device(amd, rng, name):
    """The native MultiStage model equals three scalar SparseCVIGaussianProcess models on the same inducing grid (Bernoulli on all
    points with labels 1[y = 0]; Bernoulli on y >= 1 with labels 1[y = 1]; Poisson on y >= 2 with counts y - 2): site blocks, exactly
    zero cross-latent blocks and ELBO = sum of the three, at 1e-8 over twenty damped steps.  100 inducing points, 3 000 points."""
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Bernoulli, Poisson
    from vidp_amd.multi_latent_variational import MultiLatentSparseCVI
    from vidp_amd.sparse_variational_cvi import SparseCVIGaussianProcess
    kids, _, mk, _, make = _setup(name)
    z = 0.25 * np.arange(100.0)
    t, y = make(rng, z, 3000)
    m = MultiLatentSparseCVI(K.IndependentMultiOutput(kids), dev(z), mk(), learning_rate=0.5)
    yy = y[:, 0]
    subsets = [(np.ones(len(t), bool), (yy == 0).astype(np.float64)), (yy >= 1, (yy == 1).astype(np.float64)), (yy >= 2, yy - 2.0)]
    parts = [SparseCVIGaussianProcess(k, dev(z), lik, learning_rate=0.5) for k, lik in zip(_setup(name)[0], (Bernoulli(1e-3), Bernoulli(1e-3),
                                                                                                           Poisson(1.3)))]
    pdata = [(dev(t[sel]), dev(lab[sel][:, None])) for sel, lab in subsets]
    data = (dev(t), dev(y))
    dl = [k.state_dim for k in kids]
    D, off = sum(dl), np.concatenate([[0], np.cumsum(dl)])
    mask = np_ml.slots(dl)
    cross = (mask.T @ mask) == 0
    tol = 1e-8
    for step in range(20):
        m.update_sites(data)
        total = 0.0
        n1, n2 = host(m.nat1), host(m.nat2)
        for l, (p, pd) in enumerate(zip(parts, pdata)):
            p.update_sites(pd)
            total += float(p.classic_elbo(pd))
            sl = np.r_[off[l]:off[l + 1], D + off[l]:D + off[l + 1]]
            w1, w2 = host(p.nat1), host(p.nat2)
            np.testing.assert_allclose(n1[:, sl], w1, rtol=tol, atol=tol * np.abs(w1).max())
            np.testing.assert_allclose(n2[:, sl][:, :, sl], w2, rtol=tol, atol=tol * np.abs(w2).max())
        assert np.all(n2[:, cross] == 0.0)
        np.testing.assert_allclose(float(m.elbo(data)), total, rtol=tol)
    print(f"ml decomposition {name}: elbo {float(m.elbo(data))!r} sum of the three scalar models {total!r}")
    m.dist_p.plan.check_info()


@pytest.mark.parametrize("name", ["multistage5", "hetgauss16"])
def test_step_graph_replays_equal_eager_steps(amd, rng, name):
    """`update_sites; classic_elbo` captured once: ten replays equal ten eager steps of a twin model at 1e-12 (sites relative to
    the largest entry, ELBO relative), and eager calls after the replays see the replayed sites."""
    import torch
    from vidp_amd import kernels as K
    from vidp_amd.multi_latent_variational import MultiLatentSparseCVI
    kids, _, mk, _, make = _setup(name)
    z = 0.25 * np.arange(120.0)
    t, y = make(rng, z, 3000)
    data = (dev(t), dev(y))
    new = lambda: MultiLatentSparseCVI(K.IndependentMultiOutput(kids), dev(z), mk(), learning_rate=0.5)
    a, b = new(), new()
    step = a.step_graph(data)
    assert float(a.nat1.abs().max()) == 0.0          # capturing moved nothing
    for _ in range(10):
        e = step()
        b.update_sites(data)
        eb = b.classic_elbo(data)
        torch.cuda.synchronize()
        np.testing.assert_allclose(float(e), float(eb), rtol=1e-12)
        for x, w in ((a.nat1, b.nat1), (a.nat2, b.nat2)):
            np.testing.assert_allclose(host(x), host(w), rtol=0, atol=1e-12 * float(w.abs().max()))
    np.testing.assert_allclose(float(a.classic_elbo(data)), float(eb), rtol=1e-12)
    a.dist_p.plan.check_info()
