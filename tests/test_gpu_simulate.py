"""GPU tests of the simulation feature: the counter-based normal stream (mfgm_normal_fill) against its NumPy restatement, Euler-Maruyama
(sde_utils.euler_maruyama) on the HIP kernel against the torch route, the reference's tests and the exact moments of the recursion, and
generate_data end to end."""
import numpy as np
import pytest
import torch

from tests import np_sim

pytestmark = pytest.mark.gpu

SEEDS = [0, 1, 123456789, 2 ** 32 + 17, 2 ** 64 - 1]


def host(t):
    return t.detach().cpu().numpy()


def _grid(N, dt=0.01, start=None):
    start = dt if start is None else start
    return torch.as_tensor(start + dt * np.arange(N), dtype=torch.float64, device="cuda")


# ---- 3. the stream -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("d", [1, 2, 3, 6])
def test_normal_fill_matches_the_restatement(seed, d):
    from vidp_amd.sde_utils import normal_stream
    P, K = 5, 7
    z = host(normal_stream(P, K, d, seed=seed))
    np.testing.assert_allclose(z, np_sim.normals(seed, 0, range(P), range(K), d), rtol=0, atol=1e-13)
    z1 = host(normal_stream(P, K, d, seed=seed, stream=1))
    np.testing.assert_allclose(z1, np_sim.normals(seed, 1, range(P), range(K), d), rtol=0, atol=1e-13)
    assert np.abs(z1 - z).max() > 0.1


def test_normal_fill_large_indices():
    """Path and step indices above 2^16 (every counter word carries high bits)."""
    from vidp_amd.sde_utils import normal_stream
    seed = 2 ** 40 + 3
    z = host(normal_stream(70_001, 3, 3, seed=seed))
    sel = [0, 65_535, 65_536, 70_000]
    np.testing.assert_allclose(z[sel], np_sim.normals(seed, 0, sel, range(3), 3), rtol=0, atol=1e-13)
    z = host(normal_stream(2, 70_001, 2, seed=seed))
    ks = [0, 65_536, 70_000]
    np.testing.assert_allclose(z[:, ks], np_sim.normals(seed, 0, [0, 1], ks, 2), rtol=0, atol=1e-13)


def test_normal_fill_moments_and_correlations():
    from vidp_amd.sde_utils import normal_stream
    P, K, d = 1024, 1024, 4                       # 2^22 normals
    z = normal_stream(P, K, d, seed=99)
    n = z.numel()
    v = z.reshape(-1)
    mean, var, m4 = float(v.mean()), float(v.var()), float((v ** 4).mean())
    assert abs(mean) < 5 / np.sqrt(n)
    assert abs(var - 1) < 5 * np.sqrt(2 / n)
    assert abs(m4 - 3) < 5 * np.sqrt(96 / n)
    lag_k = float((z[:, 1:] * z[:, :-1]).mean())       # consecutive steps of a path
    lag_i = float((z[1:] * z[:-1]).mean())             # neighbouring paths at a step
    lag_j = float((z[..., 1:] * z[..., :-1]).mean())   # inside a step (the cos / sin pair and across pairs)
    for c, m in ((lag_k, P * (K - 1) * d), (lag_i, (P - 1) * K * d), (lag_j, P * K * (d - 1))):
        assert abs(c) < 5 / np.sqrt(m)


# ---- 4. reproducibility --------------------------------------------------------------------------------------------------------------
def test_reproducibility_and_batch_independence():
    from vidp_amd import sde as S
    from vidp_amd.sde_utils import euler_maruyama
    sde = S.DoubleWellSDE(q=0.7 * torch.eye(2, dtype=torch.float64))
    x0 = torch.randn(300, 2, dtype=torch.float64, device="cuda")
    tg = _grid(200)
    a = euler_maruyama(sde, x0, tg, seed=11)
    b = euler_maruyama(sde, x0, tg, seed=11)
    assert torch.equal(a, b)
    for m in (1, 63, 65, 129):
        sub = euler_maruyama(sde, x0[:m], tg, seed=11)
        assert torch.equal(sub, a[:m])
    c = euler_maruyama(sde, x0, tg, seed=12)
    assert not torch.equal(c[:, 1:], a[:, 1:]) and float((c - a).abs().max()) > 0.1


# ---- 5. shapes and alignment (reference tests/unit/test_sde.py:109-144) --------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 1])
def test_euler_maruyama_shapes(B):
    from vidp_amd import sde as S
    from vidp_amd.sde_utils import euler_maruyama
    tg = torch.linspace(0.001, 1.0, 1000, dtype=torch.float64, device="cuda")
    X = euler_maruyama(S.OrnsteinUhlenbeckSDE(0.7), torch.randn(B, 1, dtype=torch.float64, device="cuda"), tg)
    assert tuple(X.shape) == (B, 1000, 1) and X.dtype == torch.float64 and X.is_cuda


@pytest.mark.parametrize("B", [3, 1])
def test_deterministic_euler_maruyama_value(B):
    from vidp_amd import sde as S
    from vidp_amd.sde_utils import euler_maruyama
    decay = -0.8
    sde = S.OrnsteinUhlenbeckSDE(decay, q=torch.eye(1, dtype=torch.float64))
    sde.q = 1e-20 * sde.q
    tg = torch.linspace(0.001, 1.0, 1000, dtype=torch.float64, device="cuda")
    x0 = torch.randn(B, 1, dtype=torch.float64, device="cuda")
    X = host(euler_maruyama(sde, x0, tg, seed=3))
    dt = float(tg[1] - tg[0])
    expect = host(x0)[:, None, :] * (1 - decay * dt) ** np.arange(1000)[None, :, None]
    np.testing.assert_allclose(X, expect, atol=1e-5)


def test_grid_from_zero_repeats_x0_and_rejections():
    from vidp_amd import sde as S
    from vidp_amd.sde_utils import euler_maruyama
    sde = S.OrnsteinUhlenbeckSDE(0.5)
    x0 = torch.randn(4, 1, dtype=torch.float64, device="cuda")
    X = euler_maruyama(sde, x0, _grid(10, start=0.0))
    assert torch.equal(X[:, 1], X[:, 0]) and torch.equal(X[:, 0], x0) and not torch.equal(X[:, 2], X[:, 1])
    with pytest.raises(ValueError):
        euler_maruyama(sde, x0, torch.tensor([0.0, 0.2, 0.1], dtype=torch.float64))
    with pytest.raises(ValueError):
        euler_maruyama(sde, x0, torch.tensor([-0.1, 0.0, 0.1], dtype=torch.float64))
    with pytest.raises(ValueError):
        euler_maruyama(sde, torch.zeros(4, 2, dtype=torch.float64, device="cuda"), _grid(5))
    with pytest.raises(ValueError):
        euler_maruyama(sde, torch.zeros(4, dtype=torch.float64, device="cuda"), _grid(5))


def test_non_uniform_grid_increment_variance():
    from vidp_amd import sde as S
    from vidp_amd.sde_utils import euler_maruyama
    q = 0.6
    sde = S.OrnsteinUhlenbeckSDE(0.0, q=q * torch.eye(1, dtype=torch.float64))
    dts = np.tile([0.01, 0.04, 0.002], 10)
    tg = torch.as_tensor(np.cumsum(dts), device="cuda")
    B = 2 ** 16
    X = euler_maruyama(sde, torch.zeros(B, 1, dtype=torch.float64, device="cuda"), tg, seed=5)
    inc = host(X[:, 1:, 0] - X[:, :-1, 0])
    ratio = inc.var(axis=0) / (q * dts[:-1])
    assert np.all(np.abs(ratio - 1) < 5 * np.sqrt(2 / B)), ratio


# ---- 6. native against torch ---------------------------------------------------------------------------------------------------------
def _q(d, full, scale=1.0):
    if not full:
        return scale * torch.diag(torch.linspace(0.5, 1.2, d, dtype=torch.float64))
    g = torch.Generator().manual_seed(d)
    A = torch.randn(d, d, generator=g, dtype=torch.float64)
    return scale * (A @ A.T / d + 0.5 * torch.eye(d, dtype=torch.float64))


def _cases():
    from vidp_amd import sde as S
    cases = []
    for d in (1, 2, 3, 6, 8):
        for full in (False, True):
            if d == 1 and full:
                continue
            cases.append((f"ou-d{d}-{'full' if full else 'diag'}", lambda q: S.OrnsteinUhlenbeckSDE(0.8, q=q), d, full))
            cases.append((f"dw-d{d}-{'full' if full else 'diag'}", lambda q: S.DoubleWellSDE(q=q, scale=1.5, c=0.7), d, full))
    for d in (1, 2, 3):
        for full in (False, True):
            if d == 1 and full:
                continue
            cases.append((f"benes-d{d}-{full}", lambda q: S.BenesSDE(1.1, q=q), d, full))
            cases.append((f"sine-d{d}-{full}", lambda q: S.SineDiffusionSDE(0.3, q=q), d, full))
            cases.append((f"sqrt-d{d}-{full}", lambda q: S.SqrtDiffusionSDE(0.9, q=q), d, full))
    cases.append(("vdp-diag", lambda q: S.VanderPolOscillatorSDE(a=2.0, tau=5.0, q=q), 2, False))
    cases.append(("vdp-full", lambda q: S.VanderPolOscillatorSDE(a=2.0, tau=5.0, q=q), 2, True))
    cases.append(("mlp", lambda q: S.MLPDrift(q=q, seed=4), 1, False))
    cases.append(("mlp-wide", lambda q: S.MLPDrift(q=q, weights=(torch.randn(1, 13, dtype=torch.float64), 0.1 * torch.randn(13, dtype=torch.float64),
                                                                 torch.randn(13, 1, dtype=torch.float64) / 4, torch.tensor([0.2], dtype=torch.float64))), 1, False))
    return cases


CASES = _cases()


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("name, make, d, full", CASES, ids=[c[0] for c in CASES])
def test_native_matches_torch_route(name, make, d, full):
    from vidp_amd.sde_utils import euler_maruyama, native_kind
    torch.manual_seed(0)
    sde = make(_q(d, full))
    assert native_kind(sde) is not None
    N = 1000
    dt = 0.002 if name.startswith("vdp") else 0.005
    tg = _grid(N, dt)
    x0 = 0.5 * torch.randn(70, d, dtype=torch.float64, device="cuda")
    a = euler_maruyama(sde, x0, tg, seed=21, native=True)
    b = euler_maruyama(sde, x0, tg, seed=21, native=False)
    assert torch.isfinite(b).all()
    assert _rel(a, b) <= 1e-11, _rel(a, b)
    # no noise: against a plain torch recursion of the drift
    sde.q = 1e-20 * sde.q
    a = euler_maruyama(sde, x0, tg, seed=21, native=True)
    x, ref = x0.clone(), [x0]
    tprev = 0.0
    for k in range(N - 1):
        dtk = float(tg[k]) - tprev
        tprev = float(tg[k])
        x = x + sde.drift(x) * dtk
        ref.append(x)
    ref = torch.stack(ref, 1)
    # what is left of the noise is sqrt(1e-20 dt) L z per step (the reference's test allows atol 1e-5 for it)
    assert _rel(a, ref) <= 1e-6, _rel(a, ref)


def test_native_matches_the_numpy_recursion():
    """The kernel against the NumPy restatement of stream and recursion (an independent check of the torch route's noise wiring)."""
    from vidp_amd import sde as S
    from vidp_amd.sde_utils import euler_maruyama
    d, B, N, seed = 3, 5, 40, 2 ** 33 + 9
    q = _q(d, True)
    sde = S.DoubleWellSDE(q=q, scale=1.5, c=0.7)
    x0 = torch.randn(B, d, dtype=torch.float64, device="cuda")
    tg = _grid(N, 0.01)
    X = host(euler_maruyama(sde, x0, tg, seed=seed))
    z = np_sim.normals(seed, 0, range(B), range(N - 1), d)
    ref = np_sim.euler_maruyama(lambda x: 1.5 * x * (0.7 - x * x), host(x0), host(tg), np.linalg.cholesky(q.numpy()), z)
    np.testing.assert_allclose(X, ref, rtol=1e-11, atol=1e-11)


# ---- 7. statistics ---------------------------------------------------------------------------------------------------------------------
def test_ou_moments_of_the_discrete_recursion():
    from vidp_amd import sde as S
    from vidp_amd.sde_utils import euler_maruyama
    lam, q, dt, N, B, x0v = 1.3, 0.8, 0.01, 501, 2 ** 16, 1.5
    sde = S.OrnsteinUhlenbeckSDE(lam, q=q * torch.eye(1, dtype=torch.float64))
    X = host(euler_maruyama(sde, torch.full((B, 1), x0v, dtype=torch.float64, device="cuda"), _grid(N, dt), seed=8))[..., 0]
    a = 1 - lam * dt
    for n in (N // 2, N - 1):
        m = a ** n * x0v
        v = q * dt * (1 - a ** (2 * n)) / (1 - a * a)
        assert abs(X[:, n].mean() - m) < 5 * np.sqrt(v / B)
        assert abs(X[:, n].var() - v) < 5 * v * np.sqrt(2 / (B - 1))


def test_increment_covariance_full_q():
    from vidp_amd import sde as S
    from vidp_amd.sde_utils import euler_maruyama
    q = torch.tensor([[0.9, 0.4], [0.4, 0.5]], dtype=torch.float64)
    dt, B, N = 0.02, 2 ** 14, 33
    sde = S.OrnsteinUhlenbeckSDE(0.0, q=q)
    X = host(euler_maruyama(sde, torch.zeros(B, 2, dtype=torch.float64, device="cuda"), _grid(N, dt), seed=4))
    inc = (X[:, 1:] - X[:, :-1]).reshape(-1, 2)
    n = inc.shape[0]
    C = inc.T @ inc / n
    Q = q.numpy() * dt
    for i in range(2):
        for j in range(2):
            se = np.sqrt((Q[i, i] * Q[j, j] + Q[i, j] ** 2) / n)
            assert abs(C[i, j] - Q[i, j]) < 5 * se, (C, Q)


# ---- 8. dispatch ---------------------------------------------------------------------------------------------------------------------
def test_dispatch():
    from vidp_amd import sde as S
    from vidp_amd.sde_utils import euler_maruyama, native_kind

    class Tilted(S.QuadratureSDE):
        def drift(self, x, t=None):
            return -0.5 * x + 0.2 * torch.sin(x.flip(-1))

    class TweakedOU(S.OrnsteinUhlenbeckSDE):         # inherits quad_kind = 12, but its drift is not the cubic one
        def drift(self, x, t=None):
            return -self.decay * x + 0.3

    tg = _grid(100)
    x0 = torch.randn(9, 2, dtype=torch.float64, device="cuda")
    for sde in (Tilted(torch.eye(2, dtype=torch.float64)), TweakedOU(0.5, q=torch.eye(2, dtype=torch.float64))):
        assert native_kind(sde) is None
        assert torch.equal(euler_maruyama(sde, x0, tg, seed=2), euler_maruyama(sde, x0, tg, seed=2, native=False))
        with pytest.raises(ValueError):
            euler_maruyama(sde, x0, tg, native=True)
    # the torch route of TweakedOU really used its own drift
    ou = S.OrnsteinUhlenbeckSDE(0.5, q=torch.eye(2, dtype=torch.float64))
    assert float((euler_maruyama(TweakedOU(0.5, q=torch.eye(2, dtype=torch.float64)), x0, tg, seed=2) - euler_maruyama(ou, x0, tg, seed=2))
                 .abs().max()) > 0.1
    # an MLP drift wider than the kernel's parameter block falls back
    nh = 14
    wide = S.MLPDrift(weights=(torch.randn(1, nh, dtype=torch.float64), torch.zeros(nh, dtype=torch.float64),
                               torch.randn(nh, 1, dtype=torch.float64) / 4, torch.zeros(1, dtype=torch.float64)))
    assert native_kind(wide) is None
    x1 = torch.randn(9, 1, dtype=torch.float64, device="cuda")
    assert torch.equal(euler_maruyama(wide, x1, tg, seed=2), euler_maruyama(wide, x1, tg, seed=2, native=False))
    with pytest.raises(ValueError):
        euler_maruyama(wide, x1, tg, native=True)
    # parameters are read at call time
    sde = S.OrnsteinUhlenbeckSDE(0.5)
    before = euler_maruyama(sde, x1, tg, seed=2, native=True)
    sde.assign("decay", 2.0)
    after = euler_maruyama(sde, x1, tg, seed=2, native=True)
    assert not torch.equal(before, after)
    assert _rel(after, euler_maruyama(S.OrnsteinUhlenbeckSDE(2.0), x1, tg, seed=2, native=False)) <= 1e-12


# ---- 9. data generation end to end ---------------------------------------------------------------------------------------------------
def test_generate_data_end_to_end(tmp_path):
    from vidp_amd import exp_io, generate_data
    from vidp_amd import sde as S
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.variational_cvi_sde import CVISitesSDE
    sigma, n = 0.2, 400
    path = generate_data.main(["-sde", "dw", "-q", "0.8", "-t0", "0", "-t1", "8", "-x0", "0.5", "-dt", "0.01", "-n", str(n), "-si",
                               str(sigma), "-o", str(tmp_path), "-s", "7", "-dim", "1"])
    z = np.load(path)
    for key in ("sde", "decay", "Q", "x0", "sigma", "latent_process", "observations", "observation_grid", "time_grid", "test_observations",
                "test_grid"):
        assert key in z.files
    assert str(z["sde"]) == "dw"
    Q, x0, noise, latent, obs, tg, test = exp_io.load_exp_data(path)
    tgh = host(tg)
    assert tgh.shape == (801,) and latent.shape == (801, 1) and noise.item() == sigma
    np.testing.assert_array_equal(latent[0], x0[0])
    og, tsg = host(obs[0]), host(test[0])
    assert og.shape == (n,) and tsg.shape == (int(0.2 * n),) and np.all(np.diff(og) > 0) and np.all(np.diff(tsg) > 0)
    assert np.isin(og, tgh).all() and np.isin(tsg, tgh).all()
    resid = host(obs[1])[:, 0] - latent[np.searchsorted(tgh, og), 0]
    assert abs(resid.std() - sigma) < 5 * sigma / np.sqrt(2 * n)
    # the latent path is the seed's Euler-Maruyama path
    from vidp_amd.sde_utils import euler_maruyama
    again = euler_maruyama(S.DoubleWellSDE(q=torch.as_tensor(Q)), torch.as_tensor(x0, device="cuda"), tg, seed=7)
    np.testing.assert_array_equal(host(again)[0], latent)
    # a CVI-DP model on the file
    d = 1
    lik = MultivariateGaussian(torch.as_tensor(noise.item() * np.eye(d), device="cuda"))
    m = CVISitesSDE(S.DoubleWellSDE(q=torch.as_tensor(Q)), tgh, (obs[0], obs[1][None]), lik, prior_initial_state=(np.zeros(d), np.eye(d)))
    for _ in range(3):
        m.update_data_sites(0.5)
        m.update_girsanov_sites(0.2)
        assert np.isfinite(float(m.classic_elbo()))
