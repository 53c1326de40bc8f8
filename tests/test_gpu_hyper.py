"""
GPU tests of the hyper-parameter score: k_kernel_score (csrc/mfgm_score.h, entry point mfgm_packed_kernel_score,
Plan.kernel_score) against the fp64 restatement tests/np_hyper.py on identical inputs for every shape of term and d = 1 .. 8, its
edges, GaussianProcessRegression.log_likelihood_and_grad against the dense-covariance gradient, the sites models against the tape and
against difference quotients, the torch fallback route, and KernelHyperTrainer.  fp64.

Tolerance of the kernel against the restatement: 10 x np_hyper.FP64_SPREAD = 6.6e-11, the worst fp64-against-long-double spread of the
same formulas measured in tests/test_host_hyper.py, relative to max(1, |g|); measured on an MI355X: worst 5.0e-12 over all cases
(the Sums with a Matern-5/2 term), 1e-16 .. 3e-13 for the other trees.
"""
import numpy as np
import pytest

from tests import np_hyper as H

pytestmark = pytest.mark.gpu

NOISE = 0.3
TOL = 10.0 * H.FP64_SPREAD


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


def set_means(k, rng):
    """A random state mean on the tree (on the children of a Sum, whose mean is theirs)."""
    if type(k).__name__ == "Sum":
        for c in k.kernels:
            set_means(c, rng)
        return
    k.set_state_mean(rng.normal(size=k.state_dim))


def gpu_moments(k, t, y, plan):
    """The packed centred pairwise moments of the GPR posterior from the GPU's own selected inverse, and their host copies."""
    import torch
    from vidp_amd._lib import FULL, SYM, VEC
    from vidp_amd.kalman_filter import KalmanFilter
    ssm = k.state_space_model(dev(t), plan=plan)
    kf = KalmanFilter(ssm, k.generate_emission_model(dev(t)), dev(y)[..., None], dev([[np.sqrt(NOISE)]]))
    _, mom, _ = kf.log_likelihood_and_moments()
    pl = ssm.plan
    pl.check_info()
    T = t.shape[-1]
    nat = (host(pl.unpack(VEC, mom["x"])), host(pl.unpack(SYM, mom["Sig"])),
           host(pl.unpack(FULL, mom["Sub"], T - 1)) if T > 1 else None)
    torch.cuda.synchronize()
    return pl, mom, nat


def check_score(pl, k, spec, jitter, gaps, mom, nat, tol=TOL):
    """Plan.kernel_score against the restatement chain by chain; absent slots exactly zero; two calls identical bits."""
    import torch
    B, T = pl.B, pl.T
    td = dev(gaps) if T > 1 else None
    g = pl.kernel_score(k._terms_struct(), td, mom["x"], mom["Sig"], mom["Sub"])
    pl.check_info()
    g2 = pl.kernel_score(k._terms_struct(), td, mom["x"], mom["Sig"], mom["Sub"])
    assert torch.equal(g, g2)
    g = host(g)
    assert g.shape == (B, 8, 3, 2)
    terms = H.terms_of(spec)
    worst = 0.0
    for b in range(B):
        ref = H.score_restatement(spec, jitter, gaps[b] if T > 1 else None, nat[0][b], nat[1][b], None if T == 1 else nat[2][b])
        full = np.zeros((8, 3, 2))
        full[:len(terms)] = ref
        present = np.zeros((8, 3, 2), dtype=bool)
        for c, term in enumerate(terms):
            for f, leaf in enumerate(term):
                present[c, f, 0] = leaf[0] != "C"
                present[c, f, 1] = True
        assert (g[b][~present] == 0.0).all()
        worst = max(worst, float(np.max(np.abs(g[b] - full) / np.maximum(1.0, np.abs(full)))))
    print(f"kernel against restatement {worst:.2e} (tolerance {tol:.1e})")
    assert worst <= tol
    return g


@pytest.mark.parametrize("name,spec,jitter", H.TREES, ids=[n for n, _, _ in H.TREES])
def test_kernel_score_matches_restatement(amd, rng, name, spec, jitter, batch_shape):
    """T = 27, a different grid per chain with gaps max(Exp(0.5 l), 0.5 l), the default plan and 5-node segments (segment boundaries,
    a ragged last segment), zero and non-zero state mean.  The moments are the GPU's own selected inverse on that grid; the gaps
    handed to the kernel and to the restatement then have two entries per chain set to exactly zero (the prior precision of a
    jitter-free model with an exactly-zero Q does not exist, so no selected inverse can be taken ON such a grid: the comparison is of
    the formulas on identical inputs, and the zero entries take the kernel's skip of an exactly-zero Q block at arbitrary moments).
    The two trees with a jitter do have a posterior on a grid with zero gaps (Q = jitter I there): for them the two zero gaps per
    chain are in the grid the model is built on, as the issue describes, so A = I, Q = jitter I meets consistent moments."""
    from vidp_amd.packed import Plan
    B, T, d = int(np.prod(batch_shape)), 27, H.state_dim(spec)
    for mean in (False, True):
        for r0 in (0, 5):
            k = H.build_vidp(spec, jitter)
            if mean:
                set_means(k, rng)
            t = np.stack([H.make_grid(rng, spec, T, zeros=2 if jitter else 0) for _ in range(B)])
            y = rng.normal(size=(B, T))
            pl, mom, nat = gpu_moments(k, t, y, Plan(B, T, d, R0=r0, device="cuda") if r0 else None)
            gaps = np.diff(t, axis=-1)
            if jitter:
                assert ((gaps == 0.0).sum(axis=-1) == 2).all()
            else:
                for b in range(B):
                    gaps[b, rng.choice(T - 1, size=2, replace=False)] = 0.0
            check_score(pl, k, spec, jitter, gaps, mom, nat)


@pytest.mark.parametrize("T,r0", [(1, 0), (2, 0), (4, 5), (5, 5), (6, 5)])
def test_kernel_score_edges(amd, rng, T, r0):
    """T = 1 (the P0 term alone, null time_deltas), T = 2, T < R0, T = R0 and T = R0 + 1, on a d = 5 Sum and a d = 4 Product."""
    from vidp_amd.packed import Plan
    for name in ("sum_m52_m32", "prod_m32_h"):
        spec, jitter = next((s, j) for n, s, j in H.TREES if n == name)
        B, d = 2, H.state_dim(spec)
        k = H.build_vidp(spec, jitter)
        t = np.stack([H.make_grid(rng, spec, T) for _ in range(B)])
        y = rng.normal(size=(B, T))
        pl, mom, nat = gpu_moments(k, t, y, Plan(B, T, d, R0=r0, device="cuda") if r0 else None)
        check_score(pl, k, spec, jitter, np.diff(t, axis=-1), mom, nat)


def test_kernel_score_all_zero_gaps(amd, rng):
    """A chain whose gaps are all exactly zero next to an ordinary one: only its initial state contributes."""
    from vidp_amd.packed import Plan
    spec, jitter = next((s, j) for n, s, j in H.TREES if n == "sum_m52_m32")
    B, T, d = 2, 13, 5
    k = H.build_vidp(spec, jitter)
    t = np.stack([H.make_grid(rng, spec, T) for _ in range(B)])
    y = rng.normal(size=(B, T))
    pl, mom, nat = gpu_moments(k, t, y, Plan(B, T, d, R0=5, device="cuda"))
    gaps = np.diff(t, axis=-1)
    gaps[0] = 0.0
    g = check_score(pl, k, spec, jitter, gaps, mom, nat)
    p0 = H.score_restatement(spec, jitter, None, nat[0][0][:1], nat[1][0][:1], None)
    assert np.max(np.abs(g[0, :2] - p0) / np.maximum(1.0, np.abs(p0))) <= TOL


# -- the models ----------------------------------------------------------------------------------------------------------------------------
def _gpr_case(rng, spec, B, T=40):
    t = np.stack([H.make_grid(rng, spec, T) for _ in range(B)])
    y = rng.normal(size=(B, T))
    return t, y


def _dense(spec, jitter, t, y):
    out = [H.dense_ll_and_grad(spec, jitter, t[b], y[b], NOISE) for b in range(len(t))]
    return sum(o[0] for o in out), sum(o[1] for o in out), sum(o[2] for o in out)


def _flat(grads):
    from vidp_amd import hyper
    return np.array([float(g) for g in hyper.flatten(grads)])


@pytest.mark.parametrize("name", ["matern32", "sum_m52_m32", "prod_m32_h"])
def test_gpr_against_dense(amd, rng, name):
    """GaussianProcessRegression.log_likelihood_and_grad against the dense oracle, T = 40, B = 3, jitter 0: ll at 1e-9 relative (the
    bound of the package's other GPR-against-oracle tests),
    the kernel gradients and noise_grad at the bound of the host comparison of the restatement with the same oracle (1.01e-10 relative
    to max(1, |g|), tests/test_host_hyper.py) plus the kernel's own tolerance.  ll equals log_likelihood() to the last bit (the same
    launches in the same order)."""
    import torch
    from vidp_amd.variational_cvi import GaussianProcessRegression
    spec, jitter = next((s, j) for n, s, j in H.TREES if n == name)
    t, y = _gpr_case(rng, spec, 3)
    m = GaussianProcessRegression((dev(t), dev(y)[..., None]), H.build_vidp(spec, jitter), dev([[np.sqrt(NOISE)]]))
    ll, grads, noise_grad = m.log_likelihood_and_grad()
    assert torch.equal(ll, m.log_likelihood())
    rl, rg, rn = _dense(spec, jitter, t, y)
    tol = 1.01e-10 + TOL
    np.testing.assert_allclose(float(ll), rl, rtol=1e-9)
    got = _flat(grads)
    err = np.max(np.abs(got - rg) / np.maximum(1.0, np.abs(rg)))
    print(f"{name}: GPR gradients against dense {err:.2e}, noise {abs(float(noise_grad) - rn) / max(1.0, abs(rn)):.2e}")
    assert err <= tol
    assert abs(float(noise_grad) - rn) <= tol * max(1.0, abs(rn))
    from vidp_amd import hyper
    for g in hyper.flatten(grads):
        assert g.dim() == 0 and g.dtype == torch.float64 and g.device.type == "cpu"
    assert noise_grad.dim() == 0 and noise_grad.device.type == "cpu"


def test_cvi_against_the_tape(amd, rng):
    """CVIGaussianProcess, Gaussian likelihood, one update_sites() at learning_rate 1 (the Gaussian-optimal sites): the kernel
    gradients of log_likelihood_and_grad against classic_elbo_tape_hyper's at 1e-6 (that route's documented accuracy on
    half-lengthscale gaps)."""
    import torch
    from vidp_amd.likelihoods import Gaussian
    from vidp_amd.variational_cvi import CVIGaussianProcess
    for name in ("matern52", "prod_m32_h"):
        spec, jitter = next((s, j) for n, s, j in H.TREES if n == name)
        t = H.make_grid(rng, spec, 40)
        y = rng.normal(size=(40, 1))
        g = CVIGaussianProcess((dev(t), dev(y)), H.build_vidp(spec, jitter), Gaussian(NOISE), learning_rate=1.0)
        g.update_sites()
        ll, grads = g.log_likelihood_and_grad()
        elbo, leaves = g.classic_elbo_tape_hyper()
        from vidp_amd import hyper
        ref = np.array([float(x) for x in torch.autograd.grad(elbo, hyper.flatten(leaves))])
        np.testing.assert_allclose(float(ll), float(g.elbo()), rtol=1e-10)
        got = _flat(grads)
        print(f"{name}: native against tape, relative {np.abs(got - ref) / np.abs(ref)}")
        np.testing.assert_allclose(got, ref, rtol=1e-6, atol=0.0)


def test_bernoulli_sites_against_differences(amd, rng):
    """Bernoulli sites after three update_sites(): d log_likelihood / d lengthscale against central differences of log_likelihood()
    with the kernel rebuilt at l +- h, h = 1e-5 l, the sites held fixed; 1e-6 relative (the quotient's own accuracy)."""
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Bernoulli
    from vidp_amd.variational_cvi import CVIGaussianProcess
    t = H.make_grid(rng, H.M32, 40)
    y = rng.choice([0.0, 1.0], size=(40, 1))
    ell, var = 1.3, 0.8
    g = CVIGaussianProcess((dev(t), dev(y)), K.Matern32(ell, var), Bernoulli(), learning_rate=0.5)
    for _ in range(3):
        g.update_sites()
    ll, grads = g.log_likelihood_and_grad()

    def at(l, v):
        g.kernel.assign_hyperparameters({"lengthscale": l, "variance": v})
        g.kernel_changed()
        return float(g.log_likelihood())
    h = 1e-5 * ell
    fd_l = (at(ell + h, var) - at(ell - h, var)) / (2 * h)
    hv = 1e-5 * var
    fd_v = (at(ell, var + hv) - at(ell, var - hv)) / (2 * hv)
    at(ell, var)
    print(f"Bernoulli sites: d/dl {float(grads['lengthscale']):.10e} quotient {fd_l:.10e}; d/dvar {float(grads['variance']):.10e} "
          f"quotient {fd_v:.10e}")
    assert abs(float(grads["lengthscale"]) - fd_l) <= 1e-6 * abs(fd_l)
    assert abs(float(grads["variance"]) - fd_v) <= 1e-6 * abs(fd_v)


def test_fallback_route(amd, rng, monkeypatch):
    """VIDP_NATIVE_SCORE=0: the torch route equals the native one on two d <= 8 trees (the tolerance of the kernel-alone test,
    relative to max(1, |g|)); a d = 9 Sum of three Matern-5/2 on the wide plan against the dense oracle at 1e-7 relative
    to max(1, |g|) -- the accuracy the wide sweeps state end to end (tests/test_gpu_wide.py: the selected inverse at 1e-8, the GPR log
    likelihood at 1e-7), which the moments inherit; the LEG kernel (d = 3) against central differences of its own log_likelihood() at 1e-6."""
    import torch
    from vidp_amd import hyper, kernels as K
    from vidp_amd.variational_cvi import GaussianProcessRegression
    chol = dev([[np.sqrt(NOISE)]])
    for name in ("sum_m52_m32", "prod_m32_h_h"):
        spec, jitter = next((s, j) for n, s, j in H.TREES if n == name)
        t, y = _gpr_case(rng, spec, 2)
        m = GaussianProcessRegression((dev(t), dev(y)[..., None]), H.build_vidp(spec, jitter), chol)
        monkeypatch.setenv("VIDP_NATIVE_SCORE", "1")
        assert hyper.native_route(m._kernel, m._kalman.prior_ssm.plan)
        a = _flat(m.log_likelihood_and_grad()[1])
        monkeypatch.setenv("VIDP_NATIVE_SCORE", "0")
        assert not hyper.native_route(m._kernel, m._kalman.prior_ssm.plan)
        b = _flat(m.log_likelihood_and_grad()[1])
        err = np.max(np.abs(a - b) / np.maximum(1.0, np.abs(a)))
        print(f"{name}: fallback against native {err:.2e}")
        assert err <= TOL
    monkeypatch.delenv("VIDP_NATIVE_SCORE")
    spec = ("Sum", [("M52", 1.3, 0.8), ("M52", 0.8, 0.6), ("M52", 2.1, 1.4)])
    t, y = _gpr_case(rng, spec, 2)
    m = GaussianProcessRegression((dev(t), dev(y)[..., None]), H.build_vidp(spec), chol)
    ll, grads, ng = m.log_likelihood_and_grad()
    rl, rg, rn = _dense(spec, 0.0, t, y)
    wide = 1e-7
    np.testing.assert_allclose(float(ll), rl, rtol=wide)
    err = np.max(np.abs(_flat(grads) - rg) / np.maximum(1.0, np.abs(rg)))
    print(f"d = 9 on the wide plan: fallback against dense {err:.2e}, noise {abs(float(ng) - rn) / max(1.0, abs(rn)):.2e}")
    assert err <= wide
    assert abs(float(ng) - rn) <= wide * max(1.0, abs(rn))
    # LEG
    N = torch.tensor([[0.9, 0.2, 0.0], [-0.1, 0.7, 0.3], [0.2, 0.0, 1.1]], dtype=torch.float64)
    R = torch.tensor([[0.0, 0.8, -0.3], [0.1, 0.0, 0.5], [0.0, -0.2, 0.0]], dtype=torch.float64)
    t = np.cumsum(np.maximum(rng.exponential(0.4, size=30), 0.3))[None]
    y = rng.normal(size=(1, 30))
    m = GaussianProcessRegression((dev(t), dev(y)[..., None]), K.LatentExponentiallyGenerated(N, R), chol)
    ll, grads, _ = m.log_likelihood_and_grad()
    for nm, M0 in (("N", N), ("R", R)):
        for (i, j) in ((0, 0), (1, 2), (2, 1)):
            def at(e):
                Mx = M0.clone()
                Mx[i, j] += e
                m._kernel.assign_hyperparameters({"N": Mx if nm == "N" else N, "R": Mx if nm == "R" else R})
                return float(m.log_likelihood())
            e = 1e-5
            fd = (at(e) - at(-e)) / (2 * e)
            print(f"LEG {nm}[{i}, {j}]: {float(grads[nm][i, j]):.10e} quotient {fd:.10e}")
            assert abs(float(grads[nm][i, j]) - fd) <= 1e-6 * abs(fd), (nm, i, j)
    m._kernel.assign_hyperparameters({"N": N, "R": R})


def test_out_of_scope_kernels_raise(amd):
    from vidp_amd import kernels as K
    from vidp_amd.variational_cvi import GaussianProcessRegression
    import torch
    t = dev(np.linspace(0.0, 1.0, 8))
    pw = K.PiecewiseKernel([K.Matern32(1.0, 1.0), K.Matern32(2.0, 1.0)], torch.tensor([0.5], dtype=torch.float64))
    m = GaussianProcessRegression((t, torch.zeros(8, 1, dtype=torch.float64, device="cuda")), pw, dev([[0.5]]))
    with pytest.raises(NotImplementedError):
        m.log_likelihood_and_grad()
    m = GaussianProcessRegression((t, torch.zeros(8, 1, dtype=torch.float64, device="cuda")), K.HarmonicOscillator(1.0, 2.0), dev([[0.5]]))
    with pytest.raises(ValueError, match="jitter"):
        m.log_likelihood_and_grad()


def _trainer_run():
    import torch
    from vidp_amd import kernels as K
    from vidp_amd.trainers import KernelHyperTrainer
    from vidp_amd.variational_cvi import GaussianProcessRegression
    ell, var, noise = 0.7, 1.5, 0.1
    t = dev(np.linspace(0.0, 20.0, 200))
    f = K.Matern32(ell, var).state_space_model(t).sample(1, seed=11)[0].reshape(200, 2)[:, :1]
    gen = torch.Generator(device="cpu").manual_seed(5)
    y = f + (noise ** 0.5) * torch.randn(200, 1, generator=gen, dtype=torch.float64).cuda()
    m = GaussianProcessRegression((t, y), K.Matern32(3 * ell, 0.3 * var), dev([[noise ** 0.5]]))
    tr = KernelHyperTrainer(m, lr=0.05)
    g0 = np.linalg.norm(_flat(m.log_likelihood_and_grad()[1]))
    losses = tr.fit(200)
    g1 = np.linalg.norm(_flat(m.log_likelihood_and_grad()[1]))
    return tr, losses, g0, g1, -float(m.log_likelihood())


def test_trainer_gpr(amd):
    """T = 200, a Matern-3/2 prior sample plus noise, started at 3 l, 0.3 sigma^2: 200 Adam steps at lr 0.05 lower the loss, bring the
    gradient norm below a tenth of the initial one, and give the identical history in two runs."""
    tr, losses, g0, g1, final = _trainer_run()
    assert len(losses) == len(tr.history) == 200 and losses[0] == tr.history[0]["loss"]
    assert tr.history[0]["hyperparameters"] == {"lengthscale": 3 * 0.7, "variance": 0.3 * 1.5}
    print(f"trainer: loss {losses[0]:.4f} -> {final:.4f}, gradient norm {g0:.3e} -> {g1:.3e}, "
          f"hyper-parameters {tr.kernel.hyperparameter_values()}")
    assert final < losses[0]
    assert g1 < 0.1 * g0
    tr2, losses2, _, _, _ = _trainer_run()
    assert losses2 == losses and tr2.history == tr.history


def test_trainer_alternates_with_site_updates(amd, rng):
    """One fit(5, site_updates=2) on a Bernoulli CVI model raises the ELBO, moves the hyper-parameters, and ends no lower than the same
    ten site updates with the kernel held fixed."""
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Bernoulli
    from vidp_amd.trainers import KernelHyperTrainer
    from vidp_amd.variational_cvi import CVIGaussianProcess
    t = np.linspace(0.0, 6.0, 60)
    y = (np.sin(2 * t) + 0.3 * rng.normal(size=60) > 0).astype(np.float64)[:, None]
    mk = lambda: CVIGaussianProcess((dev(t), dev(y)), K.Matern32(2.5, 0.4), Bernoulli(), learning_rate=0.5)
    g, fixed = mk(), mk()
    e0 = float(g.elbo())
    tr = KernelHyperTrainer(g, lr=0.05)
    losses = tr.fit(5, site_updates=2)
    e1 = float(g.elbo())
    for _ in range(10):
        fixed.update_sites()
    ef = float(fixed.elbo())
    after = g.kernel.hyperparameter_values()
    print(f"CVI trainer: ELBO {e0:.4f} -> {e1:.4f} (kernel held fixed: {ef:.4f}), hyper-parameters {after}")
    assert len(losses) == 5 and e1 > e0
    assert after["lengthscale"] != 2.5 and after["variance"] != 0.4
    assert tr.history[0]["hyperparameters"] == {"lengthscale": 2.5, "variance": 0.4}
    assert e1 >= ef


def test_trainer_variants(amd, rng):
    """The other paths of KernelHyperTrainer: learn_noise with the log transform on a GPR (the model's chol_obs_covariance follows the
    learned variance), the matrix path for the LEG kernel's N and R, and PowerExpectationPropagation (log_likelihood_and_grad against
    a difference quotient at 1e-6 relative, kernel_changed() dropping the cached prior normaliser)."""
    import torch
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Bernoulli, PEPScalarLikelihood
    from vidp_amd.pep import PowerExpectationPropagation
    from vidp_amd.trainers import KernelHyperTrainer
    from vidp_amd.variational_cvi import GaussianProcessRegression
    t = np.cumsum(np.maximum(rng.exponential(0.3, size=60), 0.2))
    y = np.sin(t)[:, None] + 0.3 * rng.normal(size=(60, 1))
    m = GaussianProcessRegression((dev(t), dev(y)), K.Matern32(2.0, 0.5), dev([[0.7]]))
    tr = KernelHyperTrainer(m, lr=0.05, learn_noise=True, transform="log")
    losses = tr.fit(20)
    assert losses[-1] < losses[0]
    assert tr.history[0]["noise_variance"] == 0.7 ** 2 and tr.history[1]["noise_variance"] != 0.7 ** 2
    assert abs(float(m._chol_obs_covariance[0, 0]) ** 2 - tr._noise_variance()) == 0.0
    assert abs(float(m._chol_obs_covariance[0, 0]) ** 2 - 0.49) > 1e-3
    # first step of Adam moves every unconstrained value by lr against the gradient's sign: log x changes by exactly -+ lr
    h0, h1 = tr.history[0], tr.history[1]
    for n in ("lengthscale", "variance"):
        assert abs(abs(np.log(h1["hyperparameters"][n] / h0["hyperparameters"][n])) - 0.05) <= 1e-6
    with pytest.raises(ValueError):
        KernelHyperTrainer(GaussianProcessRegression((dev(t), dev(y)), K.Matern32(2.0, 0.5)), learn_noise=True)
    with pytest.raises(ValueError):
        KernelHyperTrainer(m, transform="exp")
    # LEG: matrices through _Adam
    N = torch.tensor([[0.9, 0.2], [-0.1, 0.7]], dtype=torch.float64)
    R = torch.tensor([[0.0, 0.8], [0.1, 0.0]], dtype=torch.float64)
    m = GaussianProcessRegression((dev(t), dev(y)), K.LatentExponentiallyGenerated(N, R), dev([[0.7]]))
    tr = KernelHyperTrainer(m, lr=0.02)
    losses = tr.fit(5)
    got = m._kernel.hyperparameter_values()
    assert losses[-1] < losses[0]
    assert not torch.equal(got["N"], N) and not torch.equal(got["R"], R)
    assert torch.equal(tr.history[0]["hyperparameters"]["N"], N)
    # PEP
    yb = (np.sin(t) > 0).astype(np.float64)[:, None]
    ell, var = 1.3, 0.8
    p = PowerExpectationPropagation((dev(t), dev(yb)), K.Matern32(ell, var), PEPScalarLikelihood(Bernoulli()), learning_rate=0.5,
                                    alpha=0.8)
    for _ in range(3):
        p.update_sites()
    p.energy()
    assert p._norm_p is not None
    ll, grads = p.log_likelihood_and_grad()

    def at(l):
        p.kernel.assign_hyperparameters({"lengthscale": l, "variance": var})
        p.kernel_changed()
        assert p._norm_p is None and p._dist_p is None
        return float(p.log_likelihood())
    h = 1e-5 * ell
    fd = (at(ell + h) - at(ell - h)) / (2 * h)
    at(ell)
    print(f"PEP: d/dl {float(grads['lengthscale']):.10e} quotient {fd:.10e}")
    assert abs(float(grads["lengthscale"]) - fd) <= 1e-6 * abs(fd)
    assert float(p.energy()) == float(p.energy())
