"""
GPU tests of the panel sparse CVI model (vidp_amd.panel_variational_cvi.PanelSparseCVI; kernels mfgm_panel_theta /
mfgm_panel_predict_lik / mfgm_panel_site_update, csrc/mfgm_panel.h): the three kernels at d = 1 .. 8 against the NumPy sums of
tests/np_panel.py with derived rounding bounds (the packed layout restated there), run-to-run bit equality, NULL outputs, absent points
as exact zeros; the native route against the torch route and the dense NumPy model over twenty damped steps; the known answer of B
single-chain SparseCVIGaussianProcess models; the cache discipline; the not-positive-definite report.  fp64.
"""
import ctypes

import numpy as np
import pytest

from oracle import np_kernels
from tests import np_panel

pytestmark = pytest.mark.gpu

EPS = 2.3e-16          # a little above the unit roundoff of fp64 per operation, as in tests/test_gpu_ml.py
KINDS = {"bernoulli": (1, 2e-3), "poisson": (2, 1.3), "gaussian": (3, 0.4)}


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


def _sym(a):
    return 0.5 * (a + np.swapaxes(a, -1, -2))


def _case(rng, d, B, M, N):
    """Random well-conditioned pair marginals given as chain blocks per series (built as tests/test_gpu_ml._case builds them), one
    shared prior block; per row a pattern of intervals: all of the row left of z[0], all right of z[M - 1], all in one interval, or
    sorted random intervals (counts 0, 1 and more); observations with NaNs, one row all NaN; rows w, c, gradients, sites, prior
    naturals."""
    n = 2 * d
    A = rng.normal(size=(B, M + 1, n, n)) / np.sqrt(n)
    S = A @ A.transpose(0, 1, 3, 2) + 0.5 * np.eye(n)
    Sig = S[:, :M, d:, d:].copy()
    Sub = np.zeros((B, M, d, d))
    Sub[:, :M - 1] = 0.3 * S[:, 1:M, d:, :d]
    P0 = S[0, M, d:, d:].copy()
    mu, pm = rng.normal(size=(B, M, d)), 0.1 * rng.normal(size=d)
    while True:          # (at d = 1 a cross block can outweigh its two unrelated diagonal blocks: halve those until the pair is safe)
        pmu, pair = np_panel.pairs(mu, Sig, Sub, pm, P0)
        weak = np.linalg.eigvalsh(pair).min(-1) <= 0.05
        if not weak.any():
            break
        Sub[:, :M - 1][weak[:, 1:M]] *= 0.5
    idx = np.zeros((B, N), dtype=np.int64)
    for b in range(B):
        pat = b % 5 if B >= 5 else rng.integers(5)
        if pat == 1:
            idx[b] = M
        elif pat == 2:
            idx[b] = rng.integers(M + 1)
        elif pat >= 3:
            idx[b] = np.sort(rng.integers(M + 1, size=N))
    seg = np.zeros((B, M + 2), dtype=np.int32)
    for b in range(B):
        seg[b, 1:] = np.cumsum(np.bincount(idx[b], minlength=M + 1))
    y = {"gaussian": rng.normal(size=(B, N)) * 1.5, "bernoulli": rng.integers(2, size=(B, N)).astype(np.float64),
         "poisson": rng.poisson(2.0, size=(B, N)).astype(np.float64)}
    absent = rng.uniform(size=(B, N)) < 0.2
    if B > 1 or rng.integers(2):
        absent[min(B - 1, 1)] = True          # one row without observations
    for v in y.values():
        v[absent] = np.nan
    return dict(d=d, B=B, M=M, N=N, Sig=Sig, Sub=Sub, mu=mu, P0=P0, pm=pm, pmu=pmu, pair=pair, idx=idx, seg=seg, y=y, absent=absent,
                w=rng.normal(size=(B, N, n)) * (0.8 / np.sqrt(n)), c=rng.uniform(0.0, 0.2, size=(B, N)),
                g1=rng.normal(size=(B, N)), g2=-rng.uniform(0.1, 1.0, size=(B, N)), nat1=0.3 * rng.normal(size=(B, M + 1, n)),
                nat2=-_sym(rng.normal(size=(B, M + 1, n, n))), plin=rng.normal(size=(M, d)), pdiag=-_sym(rng.normal(size=(M, d, d))),
                psub=rng.normal(size=(M, d, d)))


def _struct(amd, cs):
    keep = dict(idx=dev(cs["idx"], np.int32), seg=dev(cs["seg"], np.int32), w=dev(cs["w"]), c=dev(cs["c"]), pm=dev(cs["pm"]),
                P0=dev(cs["P0"]))
    s = amd._lib.PanelData()
    s.B, s.M, s.d, s.N = cs["B"], cs["M"], cs["d"], cs["N"]
    s.idx, s.seg, s.w, s.c = (keep[k].data_ptr() for k in ("idx", "seg", "w", "c"))
    s.prior_mean, s.prior_cov = keep["pm"].data_ptr(), keep["P0"].data_ptr()
    return s, keep


SHAPES = [(M, N) for M in (1, 2, 9, 130) for N in (0, 1, 37)]
GRID = [(d, B) for d in range(1, 9) for B in (1, 3, 70)]
_gid = lambda p: f"d{p[0]}-B{p[1]}"


def test_the_large_shape_is_the_one_meant(amd):
    """B = 70, M = 130: more than 64 lanes, a lane count that is no multiple of 64, at least two levels."""
    pl = amd.Plan(70, 130, 3)
    assert 70 * pl.P > 64 and (70 * pl.P) % 64 != 0 and pl.nlevels >= 2 and pl.Lpad > 70 * pl.P


@pytest.mark.parametrize("p", GRID, ids=_gid)
def test_theta_kernel_matches_numpy_sums(amd, rng, p):
    """mfgm_panel_theta against NumPy: every entry is a sum of three terms (one of them doubled), so |got - want| <= 4 EPS sum|terms|.
    Compared twice: unpacked with Plan.unpack, and as whole packed arrays against the layout formula of tests/np_panel.py, where every
    position outside the chains (padding lanes and steps, the sub-diagonal block of the last node) is exactly 0.  M = 1 has no
    sub-diagonal.  Two launches agree bit for bit; a NULL plin is a zero prior term."""
    import torch
    from vidp_amd.packed import _ptr, _stream
    d, B = p
    lib = amd._lib.load()
    for M in (1, 2, 9, 130):
        cs = _case(rng, d, B, M, 1)
        pl = amd.Plan(B, M, d)
        ins = [dev(cs[k]) for k in ("nat1", "nat2", "plin", "pdiag", "psub")]

        def run(plin=True):
            out = [torch.full_like(pl.empty(k), 7.0) for k in (amd.VEC, amd.SYM, amd.FULL)]
            amd._lib.check(lib.mfgm_panel_theta(pl.h, _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]) if plin else None, _ptr(ins[3]), _ptr(ins[4]),
                                                _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _stream()), "mfgm_panel_theta")
            torch.cuda.synchronize()
            return out

        got, again = run(), run()
        want = np_panel.theta_sums(cs["nat1"], cs["nat2"], cs["plin"], cs["pdiag"], cs["psub"])
        nat = [host(pl.unpack(amd.VEC, got[0])), host(pl.unpack(amd.SYM, got[1])),
               host(pl.unpack(amd.FULL, got[2], M - 1)) if M > 1 else np.zeros((B, 0, d, d))]
        worst = 0.0
        for k, (kind, n_nodes) in enumerate(((0, M), (2, M), (1, M - 1))):
            w, a = want[k][:, :n_nodes], want[3 + k][:, :n_nodes]
            assert np.all(np.abs(nat[k] - w) <= 4.0 * EPS * a)
            size = got[k].numel()
            pw, pa = np_panel.pack(kind, w, pl.R, pl.P, size), np_panel.pack(kind, a, pl.R, pl.P, size)
            g = host(got[k])
            assert np.all(np.abs(g - pw) <= 4.0 * EPS * pa)
            worst = max(worst, float(np.max(np.abs(g - pw) / (4.0 * EPS * pa + 1e-300))))
            assert np.array_equal(g, host(again[k]))
        print(f"panel theta d={d} B={B} M={M}: |got - numpy| / bound {worst:.3e}")
        noprior = run(plin=False)
        zl = np_panel.theta_sums(cs["nat1"], cs["nat2"], 0.0 * cs["plin"], cs["pdiag"], cs["psub"])
        assert np.all(np.abs(host(pl.unpack(amd.VEC, noprior[0])) - zl[0]) <= 4.0 * EPS * zl[3])
        assert np.array_equal(host(noprior[1]), host(got[1]))


def _predict(amd, cs, pl, name, want=("fmu", "fvar", "ve", "g1", "g2", "vs")):
    """The six outputs on the host; buffers of outputs not asked for are passed as NULL and keep their canary 7."""
    import torch
    from vidp_amd.packed import _ptr, _stream
    s, keep = _struct(amd, cs)
    kind, param = KINDS[name] if name else (0, 0.0)
    B, M, N, d = cs["B"], cs["M"], cs["N"], cs["d"]
    size = lambda k: amd._lib.load().mfgm_packed_doubles(pl.h, k)
    x = dev(np_panel.pack(0, cs["mu"], pl.R, pl.P, size(amd.VEC)))
    Sig = dev(np_panel.pack(2, cs["Sig"], pl.R, pl.P, size(amd.SYM)))
    Sub = dev(np_panel.pack(1, cs["Sub"][:, :M - 1], pl.R, pl.P, size(amd.FULL)))
    y = dev(cs["y"][name]) if name else None
    out = {k: torch.full((B, N), 7.0, dtype=torch.float64, device="cuda") for k in ("fmu", "fvar", "ve", "g1", "g2")}
    out["vs"] = torch.full((B,), 7.0, dtype=torch.float64, device="cuda")
    q = lambda k: _ptr(out[k]) if k in want else None
    amd._lib.check(amd._lib.load().mfgm_panel_predict_lik(pl.h, ctypes.byref(s), kind, param, _ptr(y), _ptr(x), _ptr(Sig), _ptr(Sub),
                                                          q("fmu"), q("fvar"), q("ve"), q("g1"), q("g2"), q("vs"), _stream()),
                   "mfgm_panel_predict_lik")
    torch.cuda.synchronize()
    return {k: host(v) for k, v in out.items()}


@pytest.mark.parametrize("p", GRID, ids=_gid)
def test_predict_kernel_matches_numpy(amd, rng, p):
    """mfgm_panel_predict_lik on marginals packed by the NumPy layout formula.  fmu, fvar within 1e-12 of the sum of absolute terms;
    ve, g1, g2 of the three kinds against tests/np_panel.py at the device's own fmu, fvar within 1e-12 of theirs; absent points exact
    zeros (nothing is masked out: the reference holds zeros and zero scales there); ve_series within (1e-12 + 4 (N + 1) EPS) of the
    row's sum of absolute terms; kind 0 equals the prediction of the likelihood kinds bit for bit; two launches agree bit for bit;
    NULL outputs keep their canary."""
    d, B = p
    for M, N in SHAPES:
        cs = _case(rng, d, B, M, N)
        pl = amd.Plan(B, M, d)
        fmu, fvar, smu, svar = np_panel.predict_sums(cs["w"], cs["c"], cs["idx"], cs["pmu"], cs["pair"])
        plain = _predict(amd, cs, pl, None, want=("fmu", "fvar"))
        assert np.all(np.abs(plain["fmu"] - fmu) <= 1e-12 * smu) and np.all(np.abs(plain["fvar"] - fvar) <= 1e-12 * svar)
        assert all(np.all(plain[k] == 7.0) for k in ("ve", "g1", "g2", "vs"))
        if N:
            print(f"panel predict d={d} B={B} M={M} N={N}: fmu / bound {np.max(np.abs(plain['fmu'] - fmu) / (1e-12 * smu)):.3e}, "
                  f"fvar / bound {np.max(np.abs(plain['fvar'] - fvar) / (1e-12 * svar)):.3e}")
        for name in KINDS:
            got, again = _predict(amd, cs, pl, name), _predict(amd, cs, pl, name)
            assert np.array_equal(got["fmu"], plain["fmu"]) and np.array_equal(got["fvar"], plain["fvar"])
            ve, g1, g2, sc = np_panel.lik_terms(np_panel.likelihood(name, KINDS[name][1]), got["fmu"], got["fvar"], cs["y"][name])
            for k, w_, s_ in (("ve", ve, sc["ve"]), ("g1", g1, sc["g1"]), ("g2", g2, sc["g2"])):
                assert np.all(np.abs(got[k] - w_) <= 1e-12 * s_), (name, k)
                assert np.all(got[k][cs["absent"]] == 0.0)
            assert np.all(np.abs(got["vs"] - ve.sum(-1)) <= (1e-12 + 4.0 * (N + 1) * EPS) * sc["ve"].sum(-1)), name
            assert np.all(got["vs"][cs["absent"].all(-1)] == 0.0)
            for k in got:
                assert np.array_equal(got[k], again[k])
            some = _predict(amd, cs, pl, name, want=("g2", "vs"))
            assert np.array_equal(some["g2"], got["g2"]) and np.array_equal(some["vs"], got["vs"])
            assert all(np.all(some[k] == 7.0) for k in ("fmu", "fvar", "ve", "g1"))
            only = _predict(amd, cs, pl, name, want=("ve",))
            assert np.array_equal(only["ve"], got["ve"]) and np.all(only["vs"] == 7.0)


def _update(amd, cs, lr):
    import torch
    from vidp_amd.packed import _ptr, _stream
    s, keep = _struct(amd, cs)
    b = [dev(cs["g1"]), dev(cs["g2"]), dev(cs["nat1"]), dev(cs["nat2"])]
    amd._lib.check(amd._lib.load().mfgm_panel_site_update(ctypes.byref(s), _ptr(b[0]), _ptr(b[1]), lr, _ptr(b[2]), _ptr(b[3]), _stream()),
                   "mfgm_panel_site_update")
    torch.cuda.synchronize()
    return host(b[2]), host(b[3])


@pytest.mark.parametrize("p", GRID, ids=_gid)
def test_site_update_kernel_matches_numpy_sums(amd, rng, p):
    """mfgm_panel_site_update against NumPy sums: an entry is (1 - lr) old + lr sum_i g_i w_ir w_ic over at most N points, bound
    (1e-12 + 4 (N + 1) EPS) sum|terms|; empty intervals (and N = 0) equal (1 - lr) old exactly; nat2 is symmetric to the bit; two
    launches agree bit for bit."""
    d, B = p
    lr = 0.7
    for M, N in SHAPES:
        cs = _case(rng, d, B, M, N)
        w1, w2, a1, a2 = np_panel.site_sums(cs["w"], cs["idx"], cs["g1"], cs["g2"], cs["nat1"], cs["nat2"], lr)
        got, again = _update(amd, cs, lr), _update(amd, cs, lr)
        bound = 1e-12 + 4.0 * (N + 1) * EPS
        for k, (want, sc) in enumerate(((w1, a1), (w2, a2))):
            assert np.all(np.abs(got[k] - want) <= bound * sc)
            assert np.array_equal(got[k], again[k])
        cnt = np.diff(cs["seg"], axis=1)
        empty = cnt == 0
        assert np.array_equal(got[0][empty], ((1 - lr) * cs["nat1"])[empty]) and np.array_equal(got[1][empty], ((1 - lr) * cs["nat2"])[empty])
        assert np.array_equal(got[1], got[1].transpose(0, 1, 3, 2))
        if B == 70:          # every pattern of rows is present: counts 0 and "all of the row" (and 1, among many intervals)
            assert empty.any() and (N == 0 or (cnt == N).any()) and (N < 2 or M < 130 or (cnt == 1).any())


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def _setup(name):
    """(torch kernel, oracle kernel, likelihood maker, oracle likelihood, data kind); the inducing points lie 0.25 apart and no
    lengthscale exceeds 1 (tests/test_gpu_ml.py gives the reason)."""
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Bernoulli, Gaussian, Poisson
    if name == "matern32-gaussian":
        return K.Matern32(1.0, 1.0), np_kernels.Matern32(1.0, 1.0), lambda: Gaussian(0.09), np_panel.likelihood("gaussian", 0.09), "gaussian"
    if name == "matern52-poisson":
        return K.Matern52(1.0, 0.8), np_kernels.Matern52(1.0, 0.8), lambda: Poisson(1.3), np_panel.likelihood("poisson", 1.3), "poisson"
    kids = lambda m: m.Sum([m.Matern32(0.8, 0.6), m.Matern52(1.0, 0.4)])
    return kids(K), kids(np_kernels), lambda: Bernoulli(1e-3), np_panel.likelihood("bernoulli", 1e-3), "bernoulli"


@pytest.mark.parametrize("name", ["matern32-gaussian", "matern52-poisson", "sum5-bernoulli"])
def test_native_model_against_torch_route_and_numpy(amd, rng, monkeypatch, name):
    """The native route follows the torch route of the same class (VIDP_NATIVE_PANEL=0) and the dense NumPy model over twenty damped
    steps (lr = 0.5) at 1e-8: B = 5, M = 60 inducing points 0.25 lengthscales apart, N = 200 with absent points.  Then predict_f at
    new unsorted times."""
    k, ok, mk, olik, kind = _setup(name)
    B, z = 5, 0.25 * np.arange(60.0)
    t, y = np_panel.panel_data(rng, kind, z, B, 200)
    data = (dev(t), dev(y))
    a, b = (amd.PanelSparseCVI(k, dev(z), mk(), B, learning_rate=0.5) for _ in range(2))
    o = np_panel.Panel(ok, z, olik, B, learning_rate=0.5)
    assert a._native() and a.kernel.state_dim == {"matern32-gaussian": 2, "matern52-poisson": 3, "sum5-bernoulli": 5}[name]
    tol = 1e-8
    for step in range(20):
        a.update_sites(data)
        ea = host(a.elbo_per_series(data))
        monkeypatch.setenv("VIDP_NATIVE_PANEL", "0")
        assert not b._native()
        b.update_sites(data)
        eb = host(b.elbo_per_series(data))
        monkeypatch.delenv("VIDP_NATIVE_PANEL")
        o.update_sites(t, y)
        eo = o.elbo_per_series(t, y)
        for x, w1, w2 in ((a.nat1, b.nat1, o.nat1), (a.nat2, b.nat2, o.nat2)):
            np.testing.assert_allclose(host(x), host(w1), rtol=tol, atol=tol * np.abs(w2).max())
            np.testing.assert_allclose(host(x), w2, rtol=tol, atol=tol * np.abs(w2).max())
        if step in (0, 19):
            print(f"panel model {name} step {step}: elbo native {ea.sum()!r} torch {eb.sum()!r} numpy {eo.sum()!r}")
        np.testing.assert_allclose(ea, eb, rtol=tol, atol=tol)
        np.testing.assert_allclose(ea, eo, rtol=tol, atol=tol)
        np.testing.assert_allclose(float(a.classic_elbo(data)), eo.sum(), rtol=tol)
    tn = rng.uniform(z[0] - 0.5, z[-1] + 0.5, size=(B, 70))
    om, ov = o.predict_f(tn)
    fm, fv = a.predict_f(dev(tn))
    assert tuple(fm.shape) == (B, 70, 1)
    np.testing.assert_allclose(host(fm)[..., 0], om, rtol=tol, atol=tol)
    np.testing.assert_allclose(host(fv)[..., 0], ov, rtol=tol, atol=tol)
    a.dist_p.plan.check_info()


def test_panel_equals_single_chain_models_on_the_device(amd, rng):
    """The known answer: B single-chain SparseCVIGaussianProcess models, one per series with that row's present points, give the same
    sites, predict_f and per-series ELBOs at 1e-8 over twenty damped steps, and classic_elbo equals their sum."""
    from vidp_amd.sparse_variational_cvi import SparseCVIGaussianProcess
    k, _, mk, _, kind = _setup("matern52-poisson")
    B, z = 4, 0.25 * np.arange(30.0)
    t, y = np_panel.panel_data(rng, kind, z, B, 80)
    m = amd.PanelSparseCVI(k, dev(z), mk(), B, learning_rate=0.5)
    assert m._native()
    data = (dev(t), dev(y))
    present = [~np.isnan(y[b, :, 0]) for b in range(B)]
    parts = [SparseCVIGaussianProcess(k, dev(z), mk(), learning_rate=0.5) for _ in range(B)]
    pdata = [(dev(t[b][ok]), dev(y[b][ok])) for b, ok in enumerate(present)]
    tol = 1e-8
    for step in range(20):
        m.update_sites(data)
        n1, n2, eb = host(m.nat1), host(m.nat2), host(m.elbo_per_series(data))
        total = 0.0
        for b, (p, pd) in enumerate(zip(parts, pdata)):
            p.update_sites(pd)
            e = float(p.classic_elbo(pd))
            total += e
            w1, w2 = host(p.nat1), host(p.nat2)
            np.testing.assert_allclose(n1[b], w1, rtol=tol, atol=tol * np.abs(w1).max())
            np.testing.assert_allclose(n2[b], w2, rtol=tol, atol=tol * np.abs(w2).max())
            np.testing.assert_allclose(eb[b], e, rtol=tol)
        np.testing.assert_allclose(float(m.classic_elbo(data)), total, rtol=tol)
    print(f"panel known answer: elbo {float(m.classic_elbo(data))!r} sum of the {B} single-chain models {total!r}")
    tn = np.sort(rng.uniform(z[0] - 0.5, z[-1] + 0.5, size=(B, 50)), axis=1)
    fm, fv = m.predict_f(dev(tn))
    for b, p in enumerate(parts):
        wm, wv = p.posterior.predict_f(dev(tn[b]))
        np.testing.assert_allclose(host(fm)[b], host(wm), rtol=tol, atol=tol)
        np.testing.assert_allclose(host(fv)[b], host(wv), rtol=tol, atol=tol)
    m.dist_p.plan.check_info()


def test_cache_follows_the_sites_and_chain_objects(amd, rng):
    """Editing nat1 in place moves the ELBO (the cached marginals and predictions drop); dist_p and dist_q are batch-B models whose
    posterior means are the ones the ELBO was computed from."""
    k, _, mk, _, kind = _setup("matern32-gaussian")
    B, z = 3, 0.25 * np.arange(20.0)
    t, y = np_panel.panel_data(rng, kind, z, B, 40)
    m = amd.PanelSparseCVI(k, dev(z), mk(), B, learning_rate=0.5)
    data = (dev(t), dev(y))
    m.update_sites(data)
    e0 = float(m.classic_elbo(data))
    assert float(m.classic_elbo(data)) == e0 and m._pred_cache is not None
    m.nat1[1, 4, 0] += 0.5
    e1 = float(m.classic_elbo(data))
    assert e1 != e0
    p, q = m.dist_p, m.dist_q
    assert p.batch_shape == q.batch_shape == (B,) and tuple(q.marginal_means.shape) == (B, len(z), 2)
    mu = host(p.plan.unpack(amd.VEC, m._marginals()["packed"]["x"]))
    np.testing.assert_allclose(host(q.marginal_means), mu, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(host(p.marginal_means), 0.0, atol=1e-12)


def test_not_positive_definite_site_is_reported(amd, rng):
    """A site set hugely positive on series 2 makes that chain's posterior precision indefinite: Plan.check_info raises an
    ArithmeticError naming chain 2 (an arithmetic report of the factorisation, which runs to its end)."""
    k, _, mk, _, kind = _setup("matern32-gaussian")
    B, z = 4, 0.25 * np.arange(20.0)
    t, y = np_panel.panel_data(rng, kind, z, B, 40)
    m = amd.PanelSparseCVI(k, dev(z), mk(), B, learning_rate=0.5)
    data = (dev(t), dev(y))
    m.update_sites(data)
    m.classic_elbo(data)
    m.dist_p.plan.check_info()
    m.nat2[2, 7] += 1e6 * dev(np.eye(4))
    m.classic_elbo(data)
    with pytest.raises(ArithmeticError, match="chain 2") as e:
        m.dist_p.plan.check_info()
    assert e.value.location[0] == 2
