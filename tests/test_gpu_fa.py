"""
GPU tests of Gaussian-process factor analysis (vidp_amd.factor_analysis_variational; kernels mfgm_fa_predict_lik / mfgm_fa_site_update /
mfgm_fa_site_update_q, csrc/mfgm_fa.h) on the case builder of tests/test_gpu_ml.py: the kernels against NumPy sums with derived
rounding bounds, run-to-run bit equality, null-output modes, the mixed likelihoods at the device's own marginals, the site update
against mfgm_sparse_site_update[_q] on the N P materialised rows; the native route against the torch route and the dense NumPy model
of tests/np_fa.py over twenty damped steps; graph capture of the step; GaussianProcessRegression with the FactorAnalysisKernel against
the dense log marginal; loading_grad on both routes.  fp64.
"""
import ctypes

import numpy as np
import pytest

from oracle import np_kernels
from tests import np_fa
from tests.test_gpu_ml import _case as _ml_case
from tests.test_gpu_ml import _pack, dev, host

pytestmark = pytest.mark.gpu

EPS = 2.3e-16          # a little above the unit roundoff of fp64 per operation, as in tests/test_gpu_ml.py


@pytest.fixture(scope="module")
def amd():
    import torch
    import vidp_amd
    assert torch.cuda.is_available()
    vidp_amd._lib.load()
    return vidp_amd


SHAPES = [((2,), 3), ((1, 1), 1), ((2, 1, 3), 5), ((2, 2, 2), 3), ((8, 8), 2), ((16, 16), 64), ((1,) * 8, 7), ((4,) * 8, 33), ((16, 1), 4)]
_ids = lambda v: ("x".join(str(n) for n in v[0]) + f"-P{v[1]}") if isinstance(v, tuple) else str(v)
KINDS = (np_fa.GAUSSIAN, np_fa.BERNOULLI, np_fa.POISSON)
PARAMS = {np_fa.GAUSSIAN: 0.6, np_fa.BERNOULLI: 2e-3, np_fa.POISSON: 1.3}


def _case(rng, shape, wmode):
    """The case of tests/test_gpu_ml.py (160 intervals with 0, 1, 2, 7 or 300 points, full pair covariances with their smallest
    eigenvalue above 0.05) with P outputs on top: weights W [P, L] ("const") or [N, P, L] ("point"), the three kinds mixed across
    outputs, observations of each kind with about 5 % NaN and two time points whose channels are all NaN, per-output gradients
    (g1, g2) [N, P] and their fold into latent space."""
    dl, P = shape
    cs = _ml_case(rng, dl)
    L, N = cs["L"], len(cs["h"])
    W = rng.normal(size=(P, L) if wmode == "const" else (N, P, L)) * (0.7 / np.sqrt(L))
    kinds = [KINDS[(p + len(dl)) % 3] for p in range(P)]
    Y = np.zeros((N, P))
    for p, k in enumerate(kinds):
        Y[:, p] = (rng.normal(size=N) * 1.5 if k == np_fa.GAUSSIAN else rng.integers(0, 2, size=N) if k == np_fa.BERNOULLI
                   else rng.poisson(1.5, size=N))
    Y[rng.uniform(size=Y.shape) < 0.05] = np.nan
    Y[[3, N // 2]] = np.nan
    assert np.isnan(Y).all(1).sum() >= 2
    g1p, g2p = rng.normal(size=(N, P)), -rng.uniform(0.1, 1.0, size=(N, P))
    Wn = np_fa.point_weights(W, N)
    i, j = np_fa.tri(L)
    cs.update(P=P, W=W, kinds=kinds, liks=[np_fa.make_lik(k, PARAMS[k]) for k in kinds], Y=Y, g1p=g1p, g2p=g2p,
              gam1=np.einsum("np,npl->nl", g1p, Wn), gam2=np.einsum("np,npl,npk->nlk", g2p, Wn, Wn)[:, i, j])
    return cs


def _struct(amd, cs):
    keep = dict(seg=dev(cs["seg"], np.int32), h=dev(cs["h"]), c=dev(cs["c"]), w=dev(cs["W"]), pm=dev(cs["pm"]), P0=dev(cs["P0"]))
    s = amd._lib.FaData()
    s.M, s.L, s.P, s.N = cs["M"], cs["L"], cs["P"], len(cs["h"])
    for k, n in enumerate(cs["dl"]):
        s.dl[k] = n
    s.seg, s.h, s.c, s.w = (keep[k].data_ptr() for k in ("seg", "h", "c", "w"))
    s.w_stride = 0 if cs["W"].ndim == 2 else cs["P"] * cs["L"]
    s.prior_mean, s.prior_cov = keep["pm"].data_ptr(), keep["P0"].data_ptr()
    return s, keep


POINT_OUT = dict(fmu="P", fvar="P", lmu="L", lcov="LT", dm="P", dv="P", gam1="L", gam2="LT")
ORDER = ("fmu", "fvar", "lmu", "lcov", "ve", "dm", "dv", "gam1", "gam2")


def _predict(amd, cs, lik, want=ORDER):
    """The nine outputs on the host; buffers of outputs not asked for are passed as NULL and keep their sentinel 7."""
    import torch
    from vidp_amd.packed import _ptr, _stream
    s, keep = _struct(amd, cs)
    q = amd._lib.FaLik()
    if lik:
        for p, k in enumerate(cs["kinds"]):
            q.kind[p], q.param[p] = k, PARAMS[k]
    N, L = len(cs["h"]), cs["L"]
    width = dict(P=cs["P"], L=L, LT=L * (L + 1) // 2)
    b = [dev(cs["mu"]), dev(cs["Sig"]), dev(cs["Sub"])]
    y = dev(cs["Y"]) if lik else None
    out = {k: torch.full((N, width[v]), 7.0, dtype=torch.float64, device="cuda") for k, v in POINT_OUT.items()}
    out["ve"] = torch.full((cs["M"] + 1,), 7.0, dtype=torch.float64, device="cuda")
    p = [_ptr(out[k]) if k in want else None for k in ORDER]
    amd._lib.check(amd._lib.load().mfgm_fa_predict_lik(ctypes.byref(s), ctypes.byref(q), _ptr(y), _ptr(b[0]), _ptr(b[1]), _ptr(b[2]), *p,
                                                       _stream()), "mfgm_fa_predict_lik")
    torch.cuda.synchronize()
    return {k: host(v) for k, v in out.items()}


@pytest.mark.parametrize("wmode", ["const", "point"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_predict_kernel_matches_numpy_sums(amd, rng, shape, wmode):
    """mfgm_fa_predict_lik with all kinds 0 against NumPy sums: every output is a sum of n products of the inputs, so
    |got - want| <= 4 n EPS sum|terms| whatever the order of summation: n = 2 max dl for lmu, (2 max dl)^2 + 1 for lcov, those times L
    respectively L^2 for fmu / fvar.  The pair covariances are full, and here every block of them is read.  Entries whose bound is 0
    are equal exactly; two launches agree bit for bit; each NULL output is left at its sentinel and the others do not change."""
    dl, P = shape
    cs = _case(rng, shape, wmode)
    L = len(dl)
    want, sc = np_fa.predict_sums(cs["h"], cs["c"], cs["idx"], cs["pmu"], cs["pair"], dl, cs["W"])
    names = ("fmu", "fvar", "lmu", "lcov")
    got, again = _predict(amd, cs, False, want=names), _predict(amd, cs, False, want=names)
    nd = 2 * max(dl)
    for name, n in (("lmu", nd), ("lcov", nd * nd + 1), ("fmu", nd * L), ("fvar", (nd * nd + 1) * L * L)):
        bound = 4.0 * n * EPS * sc[name]
        ok = bound > 0
        err = np.max(np.abs(got[name] - want[name])[ok] / bound[ok])
        print(f"fa predict dl={dl} P={P} {wmode} {name}: |got - numpy| / bound {err:.3e}")
        assert err <= 1.0
        assert np.array_equal(got[name][~ok], want[name][~ok])
        assert np.array_equal(got[name], again[name])
    for k in ("ve", "dm", "dv", "gam1", "gam2"):
        assert np.all(got[k] == 7.0)
    for drop in names:
        rest = tuple(k for k in names if k != drop)
        some = _predict(amd, cs, False, want=rest)
        assert np.all(some[drop] == 7.0) and all(np.array_equal(some[k], got[k]) for k in rest), drop


@pytest.mark.parametrize("wmode", ["const", "point"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_predict_kernel_likelihood(amd, rng, shape, wmode):
    """The three kinds mixed across the outputs, against tests/np_fa.py evaluated at the device's own fmu, fvar: dm, dv and (P = 1) the
    per-point VE of the intervals with one point within 1e-12 of the sum of absolute terms (the bound of tests/test_gpu_lik.py);
    gam1 / gam2 within that plus 4 P EPS sum|terms|; ve_part within (1e-12 + 4 300 P EPS) sum|terms|.  NaN entries give exact zeros,
    empty intervals 0; two launches agree bit for bit; NULL outputs are not written and the others do not change."""
    dl, P = shape
    cs = _case(rng, shape, wmode)
    got, again = _predict(amd, cs, True), _predict(amd, cs, True)
    plain = _predict(amd, cs, False, want=("fmu", "fvar", "lmu", "lcov"))
    for k in ("fmu", "fvar", "lmu", "lcov"):
        assert np.array_equal(got[k], plain[k])
    want, sc = np_fa.fold(cs["liks"], got["fmu"], got["fvar"], cs["Y"], cs["W"])
    for name, rel in (("dm", 1e-12), ("dv", 1e-12), ("gam1", 1e-12 + 4.0 * P * EPS), ("gam2", 1e-12 + 4.0 * P * EPS)):
        ok = sc[name] > 0
        err = np.max(np.abs(got[name] - want[name])[ok] / (rel * sc[name][ok]))
        print(f"fa lik dl={dl} P={P} {wmode} {name}: |got - numpy| / bound {err:.3e}")
        assert err <= 1.0
        assert np.array_equal(got[name][~ok], want[name][~ok])
    nan = np.isnan(cs["Y"])
    assert nan.sum() > 0.02 * nan.size and np.all(got["dm"][nan] == 0.0) and np.all(got["dv"][nan] == 0.0)
    dark = nan.all(1)
    assert dark.sum() >= 2 and np.all(got["gam1"][dark] == 0.0) and np.all(got["gam2"][dark] == 0.0)
    part, spart = np.zeros(cs["M"] + 1), np.zeros(cs["M"] + 1)
    np.add.at(part, cs["idx"], want["ve"])
    np.add.at(spart, cs["idx"], sc["ve"])
    okp = spart > 0
    errp = np.max(np.abs(got["ve"] - part)[okp] / ((1e-12 + 4.0 * 300 * P * EPS) * spart[okp]))
    print(f"fa lik dl={dl} P={P} {wmode}: ve_part / bound {errp:.3e}")
    assert errp <= 1.0
    if P == 1:
        single = cs["cnt"] == 1
        at = cs["seg"][:-1][single]
        ok = sc["ve"][at] > 0
        err1 = np.max(np.abs(got["ve"][single] - want["ve"][at])[ok] / (1e-12 * sc["ve"][at][ok]))
        print(f"fa lik dl={dl} P=1 {wmode}: per-point VE / bound {err1:.3e}")
        assert ok.sum() > 10 and err1 <= 1.0
    assert np.all(got["ve"][~okp] == 0.0) and np.all(got["ve"][cs["cnt"] == 0] == 0.0)
    for k in got:
        assert np.array_equal(got[k], again[k], equal_nan=True)
    some = _predict(amd, cs, True, want=("gam2", "ve", "dm"))
    assert all(np.array_equal(some[k], got[k]) for k in ("gam2", "ve", "dm"))
    assert all(np.all(some[k] == 7.0) for k in ("fmu", "fvar", "lmu", "lcov", "dv", "gam1"))


def _update(amd, cs, packed, lr=0.7):
    import torch
    from vidp_amd.packed import _ptr, _stream
    s, keep = _struct(amd, cs)
    lib = amd._lib.load()
    b = [dev(cs["gam1"]), dev(cs["gam2"]), dev(cs["nat1"]), dev(_pack(cs["nat2"], cs["d"]) if packed else cs["nat2"])]
    fn = lib.mfgm_fa_site_update_q if packed else lib.mfgm_fa_site_update
    amd._lib.check(fn(ctypes.byref(s), _ptr(b[0]), _ptr(b[1]), lr, _ptr(b[2]), _ptr(b[3]), _stream()), "mfgm_fa_site_update")
    torch.cuda.synchronize()
    return host(b[2]), host(b[3])


def _update_materialised(amd, cs, packed, lr=0.7):
    """mfgm_sparse_site_update[_q] on the N P scalar data points of the materialised route: rows w_ip [2D], gradients (g1_ip, g2_ip),
    P rows per time point (the CSR offsets scale by P)."""
    import torch
    from vidp_amd.packed import _ptr, _stream
    lib = amd._lib.load()
    P, NP = cs["P"], len(cs["h"]) * cs["P"]
    w = dev(np_fa.materialised_rows(cs["h"], cs["dl"], cs["W"]).reshape(NP, -1))
    seg, c0, pm, P0 = dev(cs["seg"] * P, np.int32), dev(np.zeros(NP)), dev(cs["pm"]), dev(cs["P0"])
    sd = amd._lib.SparseData()
    sd.M, sd.d, sd.N, sd.m_lo, sd.m_hi = cs["M"], cs["d"], NP, 0, 0
    sd.seg, sd.w, sd.c, sd.prior_mean, sd.prior_cov = seg.data_ptr(), w.data_ptr(), c0.data_ptr(), pm.data_ptr(), P0.data_ptr()
    b = [dev(cs["g1p"].reshape(-1)), dev(cs["g2p"].reshape(-1)), dev(cs["nat1"]), dev(_pack(cs["nat2"], cs["d"]) if packed else cs["nat2"])]
    fn = lib.mfgm_sparse_site_update_q if packed else lib.mfgm_sparse_site_update
    amd._lib.check(fn(ctypes.byref(sd), _ptr(b[0]), _ptr(b[1]), lr, _ptr(b[2]), _ptr(b[3]), _stream()), "mfgm_sparse_site_update")
    torch.cuda.synchronize()
    return host(b[2]), host(b[3])


@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
@pytest.mark.parametrize("wmode", ["const", "point"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_site_update_kernel_matches_numpy_sums(amd, rng, shape, wmode, packed):
    """mfgm_fa_site_update / _q against NumPy sums of gam h h over at most 300 points: bound 4 301 EPS sum|terms|; the dense form is
    symmetric to the bit; empty intervals equal (1 - lr) old exactly; lr = 0 leaves the sites unchanged bit for bit; two launches
    agree bit for bit.  Against mfgm_sparse_site_update[_q] on the N P materialised rows w_ip with (g1_ip, g2_ip), of which gam is the
    fold: bound 4 (300 P + 1) EPS sum_ip |g| |w| |w| -- the latent-space folding is the same update."""
    dl, P = shape
    cs = _case(rng, shape, wmode)
    lr, d = 0.7, cs["d"]
    w1, w2, a1, a2 = np_fa.site_sums(cs["h"], cs["idx"], cs["gam1"], cs["gam2"], cs["nat1"], cs["nat2"], dl, lr)
    rows = np_fa.materialised_rows(cs["h"], dl, cs["W"])
    m1, m2 = np.zeros_like(a1), np.zeros_like(a2)
    for k in np.unique(cs["idx"]):
        sel = cs["idx"] == k
        m1[k] = np.einsum("np,npj->j", np.abs(cs["g1p"][sel]), np.abs(rows[sel]))
        m2[k] = np.einsum("np,npi,npj->ij", np.abs(cs["g2p"][sel]), np.abs(rows[sel]), np.abs(rows[sel]))
    m1, m2 = np.abs((1 - lr) * cs["nat1"]) + lr * m1, np.abs((1 - lr) * cs["nat2"]) + lr * m2
    decay = (1 - lr) * cs["nat2"]
    old2 = cs["nat2"]
    if packed:
        w2, a2, m2, decay, old2 = _pack(w2, d), _pack(a2, d), _pack(m2, d), _pack(decay, d), _pack(old2, d)
    got, again, ref = _update(amd, cs, packed), _update(amd, cs, packed), _update_materialised(amd, cs, packed)
    for k, (name, want, sc, msc) in enumerate((("nat1", w1, a1, m1), ("nat2", w2, a2, m2))):
        bound, mbound = 4.0 * 301 * EPS * sc, 4.0 * (300 * P + 1) * EPS * msc
        ok, mok = bound > 0, mbound > 0
        err = np.max(np.abs(got[k] - want)[ok] / bound[ok])
        err_ref = np.max(np.abs(got[k] - ref[k])[mok] / mbound[mok])
        print(f"fa sites dl={dl} P={P} {wmode} packed={packed} {name}: |got - numpy| / bound {err:.3e}, "
              f"|got - materialised scalar kernel| / bound {err_ref:.3e}")
        assert err <= 1.0 and err_ref <= 1.0
        assert np.array_equal(got[k][~ok], want[~ok])
        assert np.array_equal(got[k], again[k])
    empty = cs["cnt"] == 0
    assert empty.sum() > 10
    np.testing.assert_array_equal(got[0][empty], ((1 - lr) * cs["nat1"])[empty])
    np.testing.assert_array_equal(got[1][empty], decay[empty])
    if not packed:
        assert np.array_equal(got[1], got[1].transpose(0, 2, 1))
    still = _update(amd, cs, packed, lr=0.0)
    assert np.array_equal(still[0], cs["nat1"]) and np.array_equal(still[1], old2)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
P_MODEL = 6
_A0 = np.random.default_rng(5).normal(size=(2, P_MODEL, 4)) * 0.5


def _weights_np(L):
    """A(t) [N, 6, L], smooth in time."""
    return lambda t: _A0[0, :, :L] + 0.3 * np.sin(0.3 * np.asarray(t))[:, None, None] * _A0[1, :, :L]


def _weights_torch(L):
    import torch
    return lambda t: torch.from_numpy(_weights_np(L)(t.detach().cpu().numpy())).to(t.device)


def _setup(name):
    """(torch child kernels, oracle child kernels, weights for the model, weights for the oracle, kinds) of a model case.  The inducing
    points lie 0.25 apart and no lengthscale exceeds 1 (tests/test_gpu_ml.py explains why)."""
    import torch
    from vidp_amd import kernels as K
    if name == "poisson5":
        kids = lambda m: [m.Matern32(1.0, 1.0), m.Matern52(0.8, 0.7)]
        return kids(K), kids(np_kernels), torch.from_numpy(_A0[0, :, :2].copy()), _A0[0, :, :2], [np_fa.POISSON] * P_MODEL
    mixed = [KINDS[p % 3] for p in range(P_MODEL)]
    if name == "mixed9":
        kids = lambda m: [m.Matern52(1.0, 1.0), m.Matern52(0.8, 0.8), m.Matern52(0.9, 0.5)]
        return kids(K), kids(np_kernels), _weights_torch(3), _weights_np(3), mixed
    kids = lambda m: [m.Sum([m.Matern52(1.0, 0.6), m.Matern12(0.7, 0.3)]), m.Sum([m.Matern52(0.8, 0.5), m.Matern12(1.0, 0.2)]),
                      m.Sum([m.Matern52(0.9, 0.4), m.Matern12(0.6, 0.3)]), m.Sum([m.Matern52(0.7, 0.3), m.Matern12(0.9, 0.1)])]
    return kids(K), kids(np_kernels), torch.from_numpy(_A0[0].copy()), _A0[0], mixed


def _liks(kinds):
    from vidp_amd.likelihoods import Bernoulli, Gaussian, Poisson
    mk = {np_fa.GAUSSIAN: Gaussian, np_fa.BERNOULLI: Bernoulli, np_fa.POISSON: Poisson}
    if len(set(kinds)) == 1:
        return mk[kinds[0]](PARAMS[kinds[0]])
    return [mk[k](PARAMS[k]) for k in kinds]


def _data(rng, z, N, kinds):
    t = np.sort(rng.uniform(z[0] - 0.3, z[-1] + 0.3, size=N))
    Y = np.zeros((N, len(kinds)))
    for p, k in enumerate(kinds):
        f = 0.6 * np.sin(0.4 * t + p)
        Y[:, p] = (f + 0.7 * rng.normal(size=N) if k == np_fa.GAUSSIAN else (rng.uniform(size=N) < 0.5 + 0.4 * f) if k == np_fa.BERNOULLI
                   else rng.poisson(np.exp(0.5 * f)))
    Y[rng.uniform(size=Y.shape) < 0.05] = np.nan
    return t, Y


B_MODEL = {2: np.array([[0.9, -0.2], [0.3, 1.1]]), 3: np.array([[0.9, -0.2, 0.1], [0.3, 1.1, -0.1], [0.0, 0.2, 0.8]]),
           4: np.eye(4) + 0.1 * np.array([[0, 1, -1, 2], [1, 0, 2, -1], [-2, 1, 0, 1], [1, -1, 1, 0.0]])}


def _model(name, z, lr=0.5):
    from vidp_amd import kernels as K
    from vidp_amd.factor_analysis_variational import FactorAnalysisSparseCVI
    kids, _, A, _, kinds = _setup(name)
    k = K.FactorAnalysisKernel(A, kids, P_MODEL)
    k.assign_loading_matrix(B_MODEL[len(kids)])
    return FactorAnalysisSparseCVI(k, dev(z), _liks(kinds), learning_rate=lr)


@pytest.mark.parametrize("name", ["poisson5", "mixed9", "mixed16"])
def test_native_model_against_torch_route_and_numpy(amd, rng, monkeypatch, name):
    """The native route follows the torch route of the same class (VIDP_NATIVE_FA=0) and the dense NumPy model over twenty damped
    steps (lr = 0.5) at 1e-8: 400 inducing points 0.25 lengthscales apart, 3 000 time points, P = 6.  Poisson at D = 5 (dense sites,
    constant weights), mixed kinds at D = 9 (time-varying weights) and D = 16 (packed sites).  Then predict_f / predict_latents at
    new times (sorted: the kernel; shuffled: the torch route)."""
    kids, okids, _, Ao, kinds = _setup(name)
    z = 0.25 * np.arange(400.0)
    t, Y = _data(rng, z, 3000, kinds)
    data = (dev(t), dev(Y))
    a = _model(name, z)
    D = a.kernel.state_dim
    assert D == {"poisson5": 5, "mixed9": 9, "mixed16": 16}[name]
    assert a._data(data) is not None and a._packed == (D > 8)
    monkeypatch.setenv("VIDP_NATIVE_FA", "0")
    b = _model(name, z)
    assert b._data(data) is None
    monkeypatch.delenv("VIDP_NATIVE_FA")
    o = np_fa.FactorAnalysisSparseCVI(okids, z, Ao, B_MODEL[len(kids)], [np_fa.make_lik(k, PARAMS[k]) for k in kinds], learning_rate=0.5)
    tol = 1e-8
    for step in range(20):
        a.update_sites(data)
        b.update_sites(data)
        eb = float(b.elbo(data))
        o.update_sites(t, Y)
        for x, w1, w2 in ((a.nat1, b.nat1, o.nat1), (a.nat2, b.nat2, o.nat2)):
            np.testing.assert_allclose(host(x), host(w1), rtol=tol, atol=tol * np.abs(w2).max())
            np.testing.assert_allclose(host(x), w2, rtol=tol, atol=tol * np.abs(w2).max())
        ea, eo = float(a.elbo(data)), o.elbo(t, Y)
        if step in (0, 19):
            print(f"fa model {name} step {step}: elbo native {ea!r} torch {eb!r} numpy {eo!r}")
        np.testing.assert_allclose(ea, eb, rtol=tol)
        np.testing.assert_allclose(ea, eo, rtol=tol)
    tn = np.sort(rng.uniform(z[0] - 0.5, z[-1] + 0.5, size=700))
    for tt in (tn, tn[rng.permutation(len(tn))]):
        om, ov = o.predict_f(tt)
        lm, lK = o.predict_latents(tt)
        fm, fv = a.predict_f(dev(tt))
        assert tuple(fm.shape) == (700, P_MODEL)
        np.testing.assert_allclose(host(fm), om, rtol=tol, atol=tol)
        np.testing.assert_allclose(host(fv), ov, rtol=tol, atol=tol)
        gm, gK = a.predict_latents(dev(tt), full_cov=True)
        gv = a.predict_latents(dev(tt))[1]
        np.testing.assert_allclose(host(gm), lm, rtol=tol, atol=tol)
        np.testing.assert_allclose(host(gK), lK, rtol=tol, atol=tol)
        np.testing.assert_allclose(host(gv), np.diagonal(lK, axis1=-2, axis2=-1), rtol=tol, atol=tol)
    fm, fv = a.predict_f_at_data(data)
    om, ov = o.predict_f(t)
    np.testing.assert_allclose(host(fm), om, rtol=tol, atol=tol)
    np.testing.assert_allclose(host(fv), ov, rtol=tol, atol=tol)
    np.testing.assert_allclose(host(a.predict_log_density(data)), host(b.predict_log_density(data)), rtol=tol, atol=tol)
    a.dist_p.plan.check_info()


@pytest.mark.parametrize("name", ["poisson5", "mixed16"])
def test_step_graph_replays_equal_eager_steps(amd, rng, name):
    """`update_sites; classic_elbo` captured once: ten replays equal ten eager steps of a twin model at 1e-12 (sites relative to
    the largest entry, ELBO relative), and eager calls after the replays see the replayed sites."""
    import torch
    kinds = _setup(name)[4]
    z = 0.25 * np.arange(120.0)
    t, Y = _data(rng, z, 1500, kinds)
    data = (dev(t), dev(Y))
    a, b = _model(name, z), _model(name, z)
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


def test_gpr_with_the_factor_analysis_kernel(amd, rng):
    """GaussianProcessRegression((t, Y [T, 3]), FactorAnalysisKernel, chol_obs [3, 3]) through the Kalman filter with a time-varying
    emission matrix: its log likelihood equals the dense log marginal of tests/np_fa.py at rtol 1e-8.  P = 3, L = 2, T = 200."""
    import torch
    from vidp_amd import kernels as K
    from vidp_amd.variational_cvi import GaussianProcessRegression
    kids = lambda m: [m.Matern32(1.0, 1.0), m.Matern52(0.8, 0.7)]
    T_, s2 = 200, 0.3
    t = 0.2 * np.arange(T_) + rng.uniform(0.0, 0.05, size=T_)          # gaps of 0.15 .. 0.25: the prior's Q blocks stay well conditioned
    Anp = lambda tt: _weights_np(2)(tt)[:, :3]
    Y = rng.normal(size=(T_, 3))
    k = K.FactorAnalysisKernel(lambda tt: _weights_torch(2)(tt)[..., :3, :], kids(K), 3)
    k.assign_loading_matrix(B_MODEL[2])
    gpr = GaussianProcessRegression((dev(t), dev(Y)), k, np.sqrt(s2) * torch.eye(3, dtype=torch.float64, device="cuda"))
    got = float(gpr.log_likelihood())
    want = np_fa.gp_log_marginal(kids(np_kernels), t, Y, np_fa.weights(Anp, B_MODEL[2], t), s2)
    print(f"fa gpr: log likelihood {got!r} dense log marginal {want!r}")
    np.testing.assert_allclose(got, want, rtol=1e-8)


@pytest.mark.parametrize("name", ["mixed9", "mixed16"])
def test_loading_grad_native_against_torch_route(amd, rng, monkeypatch, name):
    """loading_grad from the cached predict pass of the native route against the torch route of a twin model with the same sites, at
    1e-10 of the sum of absolute terms sum_ip |A_ipk| (|dm a_l| + 2 |dv| sum_l' |W_pl'| |K_ll'|)."""
    import torch
    kinds = _setup(name)[4]
    z = 0.25 * np.arange(120.0)
    t, Y = _data(rng, z, 1500, kinds)
    data = (dev(t), dev(Y))
    a = _model(name, z)
    monkeypatch.setenv("VIDP_NATIVE_FA", "0")
    b = _model(name, z)
    assert b._data(data) is None
    monkeypatch.delenv("VIDP_NATIVE_FA")
    assert a._data(data) is not None
    for _ in range(3):
        a.update_sites(data)
    b.nat1, b.nat2 = a.nat1.clone(), a.nat2.clone()
    got, want = host(a.loading_grad(data)), host(b.loading_grad(data))
    fmu, fvar, Wn = b._predict_torch(data[0])[:3]
    _, dm, dv = b._lik_terms(fmu, fvar, data[1])
    lmu, Kf = b._latents_torch(data[0])
    sdW = dm.abs()[:, :, None] * lmu.abs()[:, None, :] + 2.0 * dv.abs()[:, :, None] * torch.einsum("npk,nlk->npl", Wn.abs(), Kf.abs())
    A = b.kernel.base_weights(data[0]).abs()
    A = A if A.dim() == 3 else A.expand(len(t), *A.shape)
    scale = host(torch.einsum("npk,npl->kl", A, sdW))
    err = np.max(np.abs(got - want) / (1e-10 * scale))
    print(f"fa loading_grad {name}: |native - torch| / (1e-10 sum|terms|) = {err:.3e}")
    L = a.latent_dim
    assert got.shape == (L, L) and np.abs(got).max() > 1e-3 and err <= 1.0
