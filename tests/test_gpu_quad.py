"""
The tensor-product Gauss-Hermite kernels (csrc/mfgm_quad.h: mfgm_quad_linearize, mfgm_quad_kl, mfgm_quad_esde,
mfgm_quad_vdp_lagrange) against the plain float64 reference tests/np_quad.py (pinned on the CPU by tests/test_host_quad.py) at the
sizes the header advertises and the suite did not run: d = 3, B > 1 chains, the 40-parameter network drift, chains longer than one
block of the sum kernel, node counts with a ragged last block, the clip options, NULL outputs, the info word and the argument checks.

Tolerances
  values (kl, E, A, b, psi, lam):  |got - want| <= 4 n EPS sum|terms|,  n the number of accumulated terms (H^d d^2 per node sum, times
      T - 1 for a chain sum, N d for the Lagrange recursion), sum|terms| from np_quad; `error / bound` is printed per case;
  gradients (g1, gd, gs, dEd*, gtheta):  rtol 1e-9 with a floor of 1e-10 x the array's largest magnitude (the figure of
      test_gpu_api.py::test_cvi_sites_sde_coupled_drifts for native against autograd); `error / tolerance` is printed.  The reference's
      own reversed-node-order self-difference, measured on every KL case of this file by tests/test_host_quad.py, is at most 2.4e-13 of
      the largest magnitude, far under a tenth of that floor, so no case is loosened;
  bit-equality claims are exact.
"""
import ctypes

import numpy as np
import pytest

from tests import np_quad
from tests.helpers import QUAD_DT as DT, QUAD_MU0 as MU0, QUAD_P0 as P0, QUAD_Q as Q, quad_kl_case, quad_theta as theta
from tests.helpers import random_quad_path

pytestmark = pytest.mark.gpu

EPS = np_quad.EPS


@pytest.fixture(scope="module")
def amd():
    import torch
    import vidp_amd
    assert torch.cuda.is_available()
    vidp_amd._lib.load()
    return vidp_amd


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(x):
    return x.detach().cpu().numpy()


def fill(amd, kind, d, th, nh=0, dt=DT, q=None, mu0=None, p0=None, clip=None):
    """mfgm_quad_drift filled by hand from include/mfgm.h (not through SDE.quad_params)."""
    q = Q[d] if q is None else q
    p0 = P0[d] if p0 is None else p0
    mu0 = MU0[:d] if mu0 is None else mu0
    prm = amd._lib.QuadDrift()
    prm.kind, prm.d, prm.nh, prm.dt = kind, d, nh, dt
    for k, v in enumerate(th):
        prm.theta[k] = float(v)
    W, Pi = np.linalg.inv(dt * q), np.linalg.inv(p0)
    k = 0
    for i in range(min(d, 3)):
        prm.mu0[i] = float(mu0[i])
        for j in range(i + 1):
            prm.W[k], prm.P0inv[k] = W[i, j], Pi[i, j]
            k += 1
    prm.logdetQp, prm.logdetP0 = float(np.linalg.slogdet(dt * q)[1]), float(np.linalg.slogdet(p0)[1])
    prm.clip_lo, prm.clip_hi = (1.0, 0.0) if clip is None else clip
    return prm


def check_value(name, got, want, tot, n):
    got, want = np.broadcast_arrays(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64))
    bound = np.broadcast_to(4.0 * n * EPS * np.asarray(tot, dtype=np.float64), want.shape)
    pos = bound > 0.0
    assert np.array_equal(got[~pos], want[~pos]), name          # no terms (a structural zero): exact
    ratio = float(np.max(np.abs(got - want)[pos] / bound[pos]))
    print(f"{name}: error / bound {ratio:.3e}")
    assert ratio <= 1.0, name


def check_grad(name, got, want):
    want = np.asarray(want)
    tol = 1e-9 * np.abs(want) + 1e-10 * np.max(np.abs(want))
    assert np.max(tol) > 0.0, name
    ratio = float(np.max(np.abs(np.asarray(got) - want) / tol))
    print(f"{name}: error / tolerance {ratio:.3e}")
    assert ratio <= 1.0, name


def bit_equal(a, b):
    import torch
    return a.shape == b.shape and bool(torch.equal(a.view(torch.int64), b.view(torch.int64)))


def test_fill_matches_quad_params(amd):
    import torch
    from vidp_amd import sde as gsde
    for d, mk in ((3, lambda q: gsde.DoubleWellSDE(q, scale=2.0, c=0.7)), (2, lambda q: gsde.VanderPolOscillatorSDE(1.3, 0.9, q))):
        s = mk(torch.from_numpy(Q[d]))
        a = s.quad_params(DT, MU0[:d], P0[d], clip=(-0.5, 0.75))
        b = fill(amd, int(s.quad_kind), d, s.quad_theta()[0], clip=(-0.5, 0.75))
        assert (a.kind, a.d, a.nh, a.dt, a.clip_lo, a.clip_hi) == (b.kind, b.d, b.nh, b.dt, b.clip_lo, b.clip_hi)
        np.testing.assert_allclose(list(a.theta), list(b.theta), rtol=0, atol=0)
        for f in ("W", "P0inv", "mu0"):
            np.testing.assert_allclose(list(getattr(a, f)), list(getattr(b, f)), rtol=1e-14)
        np.testing.assert_allclose([a.logdetQp, a.logdetP0], [b.logdetQp, b.logdetP0], rtol=1e-14)


# ---- (a), (b), (c): mfgm_quad_kl, B = 3 chains of T = 5 ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kl_case():
    """kind -> (inputs of tests/helpers.quad_kl_case, np_quad.kl on them): each reference is computed once per module."""
    done = {}

    def get(kind):
        if kind not in done:
            c = quad_kl_case(kind)
            done[kind] = (c, np_quad.kl(kind, c["th"], c["dt"], c["q"], c["mu0"], c["P0"], c["mu"], c["cov"], c["sub"], nh=c["nh"]))
        return done[kind]
    return get


def _kl_call(amd, c):
    from vidp_amd import quad
    prm = fill(amd, c["kind"], c["d"], c["th"], c["nh"])
    args = (dev(c["mu"]), dev(c["cov"]), dev(c["sub"]))
    kl, (g1, gd, gs), gth = quad.kl(prm, *args, grad=True, param_grad=True)
    return prm, args, (kl, g1, gd, gs, gth)


@pytest.mark.parametrize("kind", [11, 12, 13, 14, 15, 10])
def test_kl_parity(amd, kl_case, kind):
    """(a) d = 3, kinds 11 (nh = 4) .. 15, and (b) d = 2, kind 10: full q and P0, B = 3, T = 5; value, g1 / gd / gs and gtheta per
    chain; a value-only call and a second launch give the same bits; gd is exactly symmetric."""
    from vidp_amd import quad
    c, want = kl_case(kind)
    d, T = c["d"], c["mu"].shape[1]
    prm, args, outs = _kl_call(amd, c)
    kl, g1, gd, gs, gth = outs
    tag = f"quad_kl kind {kind} d={d}"
    check_value(tag + " kl", host(kl), want["kl"], want["abs"], 20 ** d * d * d * (T - 1))
    for name, got in (("g1", g1), ("gd", gd), ("gs", gs), ("gth", gth)):
        for b in range(c["mu"].shape[0]):
            check_grad(f"{tag} chain {b} {name}", host(got)[b], want[name][b])
    assert bit_equal(quad.kl(prm, *args), kl)
    for a, b in zip(outs, _kl_call(amd, c)[2]):
        assert bit_equal(a, b)
    assert bit_equal(gd, gd.transpose(-1, -2).contiguous())


@pytest.mark.parametrize("kind", [11, 14])
def test_kl_chains_are_independent(amd, kind):
    """(c) the B = 3 call of (a) against three B = 1 calls on the slices: every output bit-equal."""
    from vidp_amd import quad
    prm, args, outs = _kl_call(amd, quad_kl_case(kind))
    for b in range(3):
        kl, (g1, gd, gs), gth = quad.kl(prm, *(a[b:b + 1] for a in args), grad=True, param_grad=True)
        for whole, part in zip(outs, (kl, g1, gd, gs, gth)):
            assert bit_equal(whole[b:b + 1].contiguous(), part)


def test_kl_long_chain(amd, rng):
    """(d) d = 1, kind 13, B = 2, T = 300: T - 1 = 299 > 256 reaches the strided loop of the chain sum and spans several 64-thread
    blocks; value and gtheta within the rounding bound with n = 299 * 20."""
    from vidp_amd import quad
    B, T, d, kind = 2, 300, 1, 13
    mu, cov, sub = random_quad_path(rng, B, T, d)
    th = theta(kind)
    want = np_quad.kl(kind, th, DT, Q[d], MU0[:d], P0[d], mu, cov, sub)
    kl, gth = quad.kl(fill(amd, kind, d, th), dev(mu), dev(cov), dev(sub), param_grad=True)
    check_value("quad_kl kind 13 d=1 T=300 kl", host(kl), want["kl"], want["abs"], 299 * 20)
    check_value("quad_kl kind 13 d=1 T=300 gtheta", host(gth)[:, 0], want["gth"][:, 0], want["gth_abs"][:, 0], 299 * 20)
    assert np.all(host(gth)[:, 1] == 0.0)


# ---- (e) mfgm_quad_linearize ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d,N", [(11, 3, 70), (12, 3, 70), (14, 3, 70), (10, 2, 130)])
def test_linearize(amd, rng, kind, d, N):
    from vidp_amd import quad
    nh = 4 if kind == 11 else 0
    mu, cov, _ = random_quad_path(rng, 1, N, d)
    mu, cov, th = mu[0], cov[0], theta(kind, nh)
    A0, b0, Aa, ba = np_quad.linearize(kind, th, DT, mu, cov, nh=nh)
    # a window that clips some entries of A and of b and leaves others of both alone
    clip = (float(np.quantile(b0, 0.3)), float(np.quantile(A0[:, np.arange(d), np.arange(d)], 0.5)))
    A1, b1, _, _ = np_quad.linearize(kind, th, DT, mu, cov, clip=clip, nh=nh)
    for full, cl in ((A0, A1), (b0, b1)):
        assert np.any(full != cl) and np.any((full == cl) & (full != 0.0))
    n = 10 ** d * d * d
    for tag, c, wA, wb in (("", None, A0, b0), (" clipped", clip, A1, b1)):
        A, b = quad.linearize(fill(amd, kind, d, th, nh, clip=c), dev(mu), dev(cov))
        check_value(f"quad_linearize kind {kind} d={d}{tag} A", host(A), wA, Aa, n)
        check_value(f"quad_linearize kind {kind} d={d}{tag} b", host(b), wb, ba, n)


def test_linearize_no_nodes(amd):
    """N = 0 returns cleanly and writes nothing."""
    import torch
    from vidp_amd.packed import _ptr, _stream
    d = 3
    prm = fill(amd, 12, d, theta(12))
    m, c, A, b = (torch.full(s, 7.5, dtype=torch.float64, device="cuda") for s in ((1, d), (1, d, d), (1, d, d), (1, d)))
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = amd._lib.load().mfgm_quad_linearize(ctypes.byref(prm), 0, _ptr(m), _ptr(c), _ptr(A), _ptr(b), _ptr(info), _stream())
    torch.cuda.synchronize()
    assert rc == 0 and int(info.item()) == 0 and bool((A == 7.5).all()) and bool((b == 7.5).all())


# ---- (f) mfgm_quad_esde --------------------------------------------------------------------------------------------------------------
def _esde_raw(amd, prm, ins, outs):
    """The C entry point with exactly the output buffers given (None: NULL)."""
    import torch
    from vidp_amd.packed import _ptr, _stream
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = amd._lib.load().mfgm_quad_esde(ctypes.byref(prm), ins[0].shape[0], *(_ptr(x) for x in ins), *(_ptr(x) for x in outs), _ptr(info),
                                        _stream())
    torch.cuda.synchronize()
    return rc, int(info.item())


@pytest.mark.parametrize("kind,d,N,nh", [(11, 3, 70, 13), (12, 3, 70, 0), (14, 3, 70, 0), (10, 2, 65, 0)])
def test_esde(amd, rng, kind, d, N, nh):
    """E, dEdm, dEdS, dEdA, dEdb and gtheta with a full q and general A, b (kind 11: nh = 13, the 40-parameter limit); then with every
    optional output NULL except E, and with gtheta alone: E bit-equal, the buffers not handed in untouched."""
    import torch
    from vidp_amd import quad
    mu, cov, _ = random_quad_path(rng, 1, N, d)
    mu, cov, th = mu[0], cov[0], theta(kind, nh)
    A, b = 0.5 * rng.normal(size=(N, d, d)), rng.normal(size=(N, d))
    want = np_quad.esde(kind, th, Q[d], mu, cov, A, b, nh=nh)
    prm = fill(amd, kind, d, th, nh)
    assert np_quad.n_params(kind, nh) == quad.n_params(prm) and (kind != 11 or quad.n_params(prm) == amd._lib.QUAD_NTHETA)
    ins = tuple(dev(x) for x in (mu, cov, A, b))
    E, (dm, dS, dA, db), gth = quad.esde(prm, *ins, grads=True, param_grad=True)
    tag = f"quad_esde kind {kind} d={d}"
    check_value(tag + " E", host(E), want[0], want[0], 20 ** d * d * d)
    for name, got, w in zip(("dEdm", "dEdS", "dEdA", "dEdb", "gtheta"), (dm, dS, dA, db, gth), want[1:]):
        check_grad(f"{tag} {name}", host(got), w)
    assert bit_equal(dS, dS.transpose(-1, -2).contiguous())
    for keep in ((), (4,)):
        bufs = [torch.full_like(x, -77.25) for x in (dm, dS, dA, db, gth)]
        E2 = torch.empty_like(E)
        rc, info = _esde_raw(amd, prm, ins, [E2] + [x if k in keep else None for k, x in enumerate(bufs)])
        assert rc == 0 and info == 0 and bit_equal(E2, E)
        for k, x in enumerate(bufs):
            assert bit_equal(x, gth) if k in keep else bool((x == -77.25).all())


# ---- (g) mfgm_quad_vdp_lagrange ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 1])
@pytest.mark.parametrize("clip", [0.0, 0.5])
def test_vdp_lagrange(amd, rng, d, clip):
    """B = 66 chains (more than one 64-thread block), N = 7; clip = 0.5 with a few NaNs planted in each of the four gradient arrays."""
    from vidp_amd import quad
    B, N, dt = 66, 7, 0.02
    A = rng.normal(size=(B, N, d, d))
    arrs = [rng.normal(size=s) for s in ((B, N, d), (B, N, d, d), (B, N + 1, d), (B, N + 1, d, d))]
    if clip > 0:
        for a in arrs:
            flat = a.reshape(-1)
            flat[rng.choice(flat.size, 5, replace=False)] = np.nan
    psi_w, lam_w, psi_a, lam_a = np_quad.vdp_lagrange(A, *arrs, dt, clip)
    assert np.all(np.isfinite(psi_w)) and np.all(np.isfinite(lam_w))
    psi, lam = quad.vdp_lagrange(dev(A), *(dev(a) for a in arrs), dt, clip=clip)
    psi, lam = host(psi), host(lam)
    assert np.array_equal(psi[:, N - 1], np.broadcast_to(1e-10 * np.eye(d), (B, d, d))) and np.all(lam[:, N - 1] == 0.0)
    check_value(f"quad_vdp_lagrange d={d} clip={clip} psi", psi, psi_w, psi_a, N * d)
    check_value(f"quad_vdp_lagrange d={d} clip={clip} lam", lam, lam_w, lam_a, N * d)


# ---- (h) error reporting -------------------------------------------------------------------------------------------------------------
def test_not_positive_definite_is_reported(amd, rng):
    """One indefinite Sig block in chain 1 of 3: kl, linearize and esde raise ArithmeticError; read with check=False, the other
    chains' numbers are those of the clean call."""
    from vidp_amd import quad
    B, T, d, kind = 3, 5, 3, 13
    mu, cov, sub = random_quad_path(rng, B, T, d)
    bad = cov.copy()
    bad[1, 2] = np.diag([0.3, -0.2, 0.25])
    prm = fill(amd, kind, d, theta(kind))
    A, b = dev(0.5 * rng.normal(size=(B, T, d, d))), dev(rng.normal(size=(B, T, d)))
    calls = {"kl": lambda c, **k: quad.kl(prm, dev(mu), dev(c), dev(sub), **k),
             "linearize": lambda c, **k: quad.linearize(prm, dev(mu), dev(c), **k)[0],
             "esde": lambda c, **k: quad.esde(prm, dev(mu), dev(c), A, b, **k)[0]}
    for name, call in calls.items():
        with pytest.raises(ArithmeticError):
            call(bad)
        got, clean = call(bad, check=False), call(cov)
        for ch in (0, 2):
            assert np.all(np.isfinite(host(got[ch]))) and bit_equal(got[ch].contiguous(), clean[ch].contiguous()), name


def test_argument_checks(amd, rng):
    """The C entry points return non-zero and launch nothing for a drift block or a set of pointers outside the interface."""
    import torch
    from vidp_amd.packed import _ptr, _stream
    lib = amd._lib.load()
    B, T = 2, 4
    z = lambda *s: torch.full(s, 3.25, dtype=torch.float64, device="cuda")
    # buffers sized for d = 4, nh = 14: larger than anything a (refused) call could describe
    mu, Sig, Sub, kl, g1, gd, gs, gth = z(B, T, 4), z(B, T, 4, 4), z(B, T - 1, 4, 4), z(B), z(B, T, 4), z(B, T, 4, 4), z(B, T - 1, 4, 4), z(B * T, 43)
    E = z(B * T)
    scratch = z(B * T * (1 + 8 + 48 + 43) + B)
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    outs = (kl, g1, gd, gs, gth, E)

    def run_kl(prm, T_=T, g1_=g1, gd_=gd, gs_=gs, gth_=gth):
        rc = lib.mfgm_quad_kl(ctypes.byref(prm), B, T_, _ptr(mu), _ptr(Sig), _ptr(Sub), _ptr(kl), _ptr(g1_), _ptr(gd_), _ptr(gs_), _ptr(gth_),
                              _ptr(scratch), _ptr(info), _stream())
        torch.cuda.synchronize()
        return rc

    def run_all(prm):
        n = B * T
        rcs = [run_kl(prm),
               lib.mfgm_quad_linearize(ctypes.byref(prm), n, _ptr(mu), _ptr(Sig), _ptr(gd), _ptr(g1), _ptr(info), _stream()),
               lib.mfgm_quad_esde(ctypes.byref(prm), n, _ptr(mu), _ptr(Sig), _ptr(Sig), _ptr(mu), _ptr(E), _ptr(g1), _ptr(gd), _ptr(gs),
                                  None, _ptr(gth), _ptr(info), _stream())]
        torch.cuda.synchronize()
        return rcs

    ok = lambda: int(info.item()) == 0 and all(bool((x == 3.25).all()) for x in outs + (scratch,))
    bad = [fill(amd, 12, 3, theta(12)), fill(amd, 10, 3, theta(10)), fill(amd, 11, 3, np.zeros(40), nh=14), fill(amd, 11, 3, np.zeros(40), nh=0),
           fill(amd, 9, 3, theta(12)), fill(amd, 16, 3, theta(12))]
    bad[0].d = 4
    for prm in bad:
        assert all(rc != 0 for rc in run_all(prm)) and ok(), (prm.kind, prm.d, prm.nh)
    good = fill(amd, 12, 3, theta(12))
    assert run_kl(good, gd_=None) != 0 and ok()                                   # gd NULL with g1 set
    assert run_kl(good, g1_=None, gd_=None, gs_=None) != 0 and ok()               # gtheta without g1
    assert run_kl(good, T_=1) != 0 and ok()
    assert lib.mfgm_quad_vdp_lagrange(B, T - 1, 4, 0.1, 0.0, _ptr(Sig), _ptr(mu), _ptr(Sig), _ptr(mu), _ptr(Sig), _ptr(gd), _ptr(g1), _stream()) != 0
    torch.cuda.synchronize()
    assert ok()


# ---- (i) the models at d = 3 -----------------------------------------------------------------------------------------------------------
def test_cvi_sites_sde_quadrature_d3(amd, rng):
    """CVISitesSDEQuadrature with a double-well drift and a full 3 x 3 diffusion matrix, T = 12, B = 2 trajectories: the HIP route
    against the same class on its torch route at the tolerances of test_gpu_api.py::test_cvi_sites_sde_coupled_drifts -- linearised
    prior 1e-12, KL 1e-12, its gradient 1e-9 (floor 1e-10 of the scale), the ELBO 1e-7 over two damped update pairs and a
    re-linearisation."""
    import torch
    from tests.helpers import assert_close
    from vidp_amd import sde as gsde
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.variational_cvi_sde import CVISitesSDEQuadrature
    T, d, B, dt = 12, 3, 2, 0.05
    grid = np.arange(T) * dt
    idx = np.array([3, 7, 10])
    y = rng.normal(size=(B, len(idx), d))
    cholR = 0.4 * np.eye(d)
    init = (np.zeros(d), 0.8 * np.eye(d))
    mk = lambda: CVISitesSDEQuadrature(gsde.DoubleWellSDE(torch.from_numpy(Q[3]), scale=2.0, c=0.7), grid, (grid[idx], dev(y)),
                                       MultivariateGaussian(dev(cholR)), prior_initial_state=init)
    g, gt = mk(), mk()
    assert g.native
    gt.native = False
    gt.set_linearized_prior()
    assert_close(host(g.dist_p.state_transitions), host(gt.dist_p.state_transitions), rtol=1e-12)
    assert_close(host(g.dist_p.state_offsets), host(gt.dist_p.state_offsets), rtol=1e-12)
    for m in (g, gt):
        m.update_data_sites(0.5)
    np.testing.assert_allclose(host(g.KL_q_p()), host(gt.KL_q_p()), rtol=1e-12)
    _, (g1, gd, gs) = g.grad_kl_wrt_exp_param()
    _, (t1, td, ts) = gt.grad_kl_wrt_exp_param()
    un = lambda m_, a, b_, c: (host(m_.plan.unpack(amd.VEC, a)), host(m_.plan.unpack(amd.SYM, b_)), host(m_.plan.unpack(amd.FULL, c, T - 1)))
    for a_, b_ in zip(un(g, g1, gd, gs), un(gt, t1, td, ts)):
        assert_close(a_, b_, rtol=1e-9, scale_atol=1e-10)
    for it in range(2):
        for m in (g, gt):
            m.update_girsanov_sites(0.2)
            m.update_data_sites(0.4)
        np.testing.assert_allclose(host(g.classic_elbo_per_trajectory()), host(gt.classic_elbo_per_trajectory()), rtol=1e-7)
        if it == 0:
            g.relinearize()
            gt.relinearize()
            np.testing.assert_allclose(host(g.classic_elbo_per_trajectory()), host(gt.classic_elbo_per_trajectory()), rtol=1e-7)
    g.plan.check_info()


def test_variational_markov_gp_quadrature_d3(amd, rng):
    """VariationalMarkovGPQuadrature at d = 3 (tanh drift, full q, T = 12): E_sde, its gradients and the Lagrange sweep against np_quad,
    before and after a parameter update (the first pass has A = b = 0; the prior's initial mean is not 0, where tanh's symmetry would make
    dE/dm vanish)."""
    import torch
    from vidp_amd import sde as gsde
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.vi_sde import VariationalMarkovGPQuadrature
    T, d, dt = 12, 3, 0.05
    N = T - 1
    grid = np.arange(T) * dt
    idx = np.array([3, 7, 10])
    y = rng.normal(size=(1, len(idx), d))
    g = VariationalMarkovGPQuadrature((grid[idx], dev(y)), gsde.BenesSDE(1.3, torch.from_numpy(Q[3])), grid, MultivariateGaussian(dev(0.5 * np.eye(d))),
                                      prior_initial_state=(np.array([0.4, -0.3, 0.2]), 0.6 * np.eye(d)), stabilize_system=False)
    for it in range(2):
        mS = g._forward_packed()
        m, S = (host(x)[0] for x in g._natural(mS))
        A, b = host(g.A)[0], host(g.b)[0]
        E, dm, dS, _, _, _ = np_quad.esde(13, [1.3, 0.0], Q[3], m[:N], S[:N], A, b)
        check_value(f"VariationalMarkovGPQuadrature d=3 pass {it} E_sde", float(g.E_sde(mS)[0]), E.sum() * dt, E.sum() * dt, 20 ** d * d * d * N)
        gm, gS = g._grad_E_sde(mS)
        check_grad(f"VariationalMarkovGPQuadrature d=3 pass {it} dEdm", host(gm)[0], dm)
        check_grad(f"VariationalMarkovGPQuadrature d=3 pass {it} dEdS", host(gS)[0], dS)
        g.update_lagrange(mS)
        dobsm, dobsS = g._jump_arrays(*g._natural(mS))
        psi, lam, psi_a, lam_a = np_quad.vdp_lagrange(A[None], host(gm), host(gS), host(dobsm), host(dobsS), dt, clip=0.0)    # not stabilised
        check_value(f"VariationalMarkovGPQuadrature d=3 pass {it} psi", host(g.psi_lagrange), psi, psi_a, N * d)
        check_value(f"VariationalMarkovGPQuadrature d=3 pass {it} lam", host(g.lambda_lagrange), lam, lam_a, N * d)
        g.update_param(mS, lr=0.3)
