"""
GPU tests of the sparse-CVI hyper-parameter gradient: k_sparse_cond_score (csrc/mfgm_sparse_score.h, entry point
mfgm_sparse_cond_score) against the np.longdouble restatement tests/np_sparse_hyper.conditional_score on identical inputs for every
block size, SparseCVIGaussianProcess.elbo_and_grad against the fp64 restatement of the whole gradient and against difference quotients
of the model's own bound, the torch route, the fixed point, what is out of scope, kernel_changed() and KernelHyperTrainer.  fp64.

Measured on an MI355X: kernel against long double worst 2.1e-14 of the absolute sum (bound 5e-12); elbo_and_grad against the
restatement 2.5e-16 (bound) and 8.5e-16 / 2.0e-15 (gradients, d <= 8 / wide; bounds 1e-8 / 1e-7); Bernoulli against difference
quotients 3.3e-10 (bound 1e-6); torch route against the HIP route 3.2e-16 (bound 5e-12).
"""
import ctypes

import numpy as np
import pytest

from tests import np_hyper as H
from tests import np_sparse_hyper as S

pytestmark = pytest.mark.gpu

KERNEL_TOL = 5e-12        # of the sum of the absolute per-point contributions to a slot: the kernel bound of DESIGN 18
GRAD_TOL, GRAD_TOL_WIDE, ELBO_TOL = 1e-8, 1e-7, 1e-9
TREES = {name: (spec, jitter) for name, spec, jitter in H.TREES}
SUM9 = ("Sum", [("M52", 1.3, 0.8), ("M52", 0.8, 0.6), ("M52", 2.1, 1.4)])
LIK = {"gaussian": ("gaussian", 0.3), "poisson": ("poisson", 0.7)}


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


def flat(grads):
    from vidp_amd import hyper
    return np.array([float(g) for g in hyper.flatten(grads)])


def rel(got, ref):
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))


# ---- 1. the kernel alone ------------------------------------------------------------------------------------------------------------------
# every block size 1, 2, 3, 4, 6, 8, the d = 8 Sum (3 + 3 + 2), and a term whose 1 x 1 factor the device moves behind the 2 x 2 one
KERNEL_TREES = ["matern12", "matern32", "matern52", "prod_m32_h", "prod_m52_h", "prod_m32_h_h", "sum_m52_m52_m32"]
# (the last tree's harmonic x constant structure has terms without process noise: it exists with a jitter only)
KERNEL_CASES = [(t, j) for t in KERNEL_TREES for j in (0.0, 1e-6)] + [("sum_prod_m12_h_const", 1e-6)]
M_K = 5


def _kernel_times(rng, spec, N):
    """Inducing points and N sorted data points: both end intervals hold points, interval 2 is empty, two points share one time, one
    point sits exactly on an inducing point; every other gap is at least half the tree's shortest time scale."""
    lm = H.shortest_lengthscale(spec)
    z = np.cumsum(rng.uniform(2.0, 3.0, M_K) * lm)
    if N == 1:
        return z, np.array([z[1] + 0.7 * lm])
    cells = np.concatenate([[z[0] - 2.0 * lm], z, [z[-1] + 2.0 * lm]])
    k = rng.choice([0, 1, 3, 4, 5], N - 2)
    k[:4] = (0, 0, 5, 5)
    lo, hi = cells[k] + 0.5 * lm, cells[k + 1] - 0.5 * lm
    t = lo + rng.uniform(0, 1, N - 2) * (hi - lo)
    t = np.sort(np.concatenate([t, [t[7]], [z[3]]]))
    return z, t


def _pair_chain(rng, M, d):
    """Random chain marginals mu [M, d], Sig [M, d, d], Sub [M, d, d] (Sigma_{t+1,t} at t) with every pair covariance positive definite."""
    n = 2 * d
    A = rng.normal(size=(M + 1, n, n)) / np.sqrt(n)
    Sfull = A @ A.transpose(0, 2, 1) + 0.5 * np.eye(n)
    Sig = Sfull[:M, d:, d:].copy()
    Sub = np.zeros((M, d, d))
    Sub[:M - 1] = 0.3 * Sfull[1:M, d:, :d]
    return rng.normal(size=(M, d)), Sig, Sub


@pytest.mark.parametrize("N", [1, 70])
@pytest.mark.parametrize("tree,jitter", KERNEL_CASES, ids=[f"{t}-{j:g}" for t, j in KERNEL_CASES])
def test_cond_score_kernel_against_long_double(amd, rng, tree, jitter, N):
    """mfgm_sparse_cond_score through the C ABI against the np.longdouble restatement on identical inputs, M = 5, N = 1 and 70 (a
    wavefront that is not full), jitter 0 and 1e-6, random a, b < 0 and positive definite pair moments.  Bound: 5e-12 of the sum of the
    absolute per-point contributions to the slot; absent slots exactly zero; identical bits on a second call."""
    import torch
    spec = TREES[tree][0]
    d = H.state_dim(spec)
    z, t = _kernel_times(rng, spec, N)
    idx, glo, ghi = S.gaps(t, z)
    if N > 1:
        assert (idx == 0).sum() >= 2 and (idx == M_K).sum() >= 2 and (idx == 2).sum() == 0 and (ghi == 0.0).sum() == 1
        assert (np.diff(t) == 0.0).sum() == 1
    w, c = S.conditional_stats(spec, jitter, glo, ghi, np.float64)
    a, b = rng.normal(size=N), -rng.uniform(0.1, 1.0, N)
    mu, Sig, Sub = _pair_chain(rng, M_K, d)
    P0 = S.transition(spec, jitter, 0.0, np.float64)[2] + jitter * np.eye(d)
    # the reference: pair moments per interval, the cotangent of w and the reverse mode in long double
    ld = np.longdouble
    mp, Sp = np.zeros((M_K + 1, 2 * d), dtype=ld), np.zeros((M_K + 1, 2 * d, 2 * d), dtype=ld)
    for m in range(M_K + 1):
        Sp[m, :d, :d] = Sig[m - 1] if m > 0 else P0
        Sp[m, d:, d:] = Sig[m] if m < M_K else P0
        if m > 0:
            mp[m, :d] = mu[m - 1]
        if m < M_K:
            mp[m, d:] = mu[m]
        if 0 < m < M_K:
            Sp[m, d:, :d], Sp[m, :d, d:] = Sub[m - 1], Sub[m - 1].T
    wl = w.astype(ld)
    wbar = a.astype(ld)[:, None] * mp[idx] + 2.0 * b.astype(ld)[:, None] * np.einsum("ijk,ik->ij", Sp[idx], wl)
    per = S.conditional_score(spec, jitter, glo, ghi, idx, M_K, a, b, wbar, wl, dtype=ld)
    ref, scale = per.sum(0), np.abs(per).sum(0)
    # the device
    k = H.build_vidp(spec, jitter)
    seg = np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=M_K + 1))]).astype(np.int32)
    keep = [dev(seg, np.int32), dev(w), dev(c), dev(np.zeros(d)), dev(P0)]
    sd = amd._lib.SparseData()
    sd.M, sd.d, sd.N, sd.m_lo, sd.m_hi = M_K, d, N, 0, 0
    sd.seg, sd.w, sd.c, sd.prior_mean, sd.prior_cov = (x.data_ptr() for x in keep)
    lib = amd._lib.load()
    args = [dev(glo), dev(ghi), dev(a), dev(b), dev(mu), dev(Sig), dev(Sub)]
    ws = torch.empty(int(lib.mfgm_sparse_cond_score_workspace_doubles(N)), dtype=torch.float64, device="cuda")
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    kt = k._terms_struct()
    out = []
    for _ in range(2):
        score = torch.full((8, 3, 2), np.nan, dtype=torch.float64, device="cuda")
        rc = lib.mfgm_sparse_cond_score(ctypes.byref(sd), ctypes.byref(kt), *[x.data_ptr() for x in args], score.data_ptr(), ws.data_ptr(),
                                        info.data_ptr(), None)
        assert rc == 0
        out.append(score)
    torch.cuda.synchronize()
    assert int(info.item()) == 0
    assert torch.equal(out[0], out[1])
    g = host(out[0])
    nt = ref.shape[0]
    present = np.zeros((8, 3, 2), dtype=bool)
    for ci, term in enumerate(H.terms_of(spec)):
        for f, leaf in enumerate(term):
            present[ci, f] = True
    assert (g[~present] == 0.0).all()
    err = np.abs(g[:nt] - ref.astype(np.float64))[present[:nt]] / np.maximum(scale.astype(np.float64), 1e-300)[present[:nt]]
    err = err[scale.astype(np.float64)[present[:nt]] > 0]
    print(f"{tree} jitter {jitter} N {N}: kernel against long double {err.max():.2e} of the absolute sum (bound {KERNEL_TOL:.0e})")
    assert err.max() <= KERNEL_TOL


# ---- 2. the model ---------------------------------------------------------------------------------------------------------------------------
M_M, N_M = 12, 40


def _model(amd, rng, spec, jitter, lik, lr=0.5, steps=2, M=M_M, N=N_M):
    """(model, data, restatement) after `steps` update_sites at learning rate lr."""
    from vidp_amd.likelihoods import Gaussian, Poisson
    from vidp_amd.sparse_variational_cvi import SparseCVIGaussianProcess
    z, t, y = S.make_problem(rng, spec, M, N, lik)
    mk = Gaussian(LIK[lik][1]) if lik == "gaussian" else Poisson(LIK[lik][1])
    m = SparseCVIGaussianProcess(H.build_vidp(spec, jitter), dev(z), mk, learning_rate=lr)
    data = (dev(t), dev(y[:, None]))
    for _ in range(steps):
        m.update_sites(data)
    return m, data, S.SparseChain(spec, jitter, z, t, y, LIK[lik])


MODEL_CASES = [("matern52", TREES["matern52"], GRAD_TOL), ("sum_m52_m32", TREES["sum_m52_m32"], GRAD_TOL),
               ("prod_m32_h", TREES["prod_m32_h"], GRAD_TOL), ("sum9_wide", (SUM9, 0.0), GRAD_TOL_WIDE)]


@pytest.mark.parametrize("lik", ["gaussian", "poisson"])
@pytest.mark.parametrize("name,tree,tol", MODEL_CASES, ids=[c[0] for c in MODEL_CASES])
def test_elbo_and_grad_against_restatement(amd, rng, name, tree, tol, lik):
    """elbo_and_grad after two update_sites at lr = 0.5 against the fp64 restatement evaluated at the model's own sites, M = 12, N = 40:
    the bound at 1e-9 relative, the gradients at 1e-8 relative to max(1, |g|) on the d <= 8 plans and at 1e-7 for the d = 9 Sum of three
    Matern-5/2 on the wide plan (torch route) -- the end-to-end accuracies tests/test_gpu_hyper.py states for the two plan families."""
    from vidp_amd import hyper
    spec, jitter = tree
    m, data, ref = _model(amd, rng, spec, jitter, lik)
    assert hyper.sparse_native_route(m, m._data(data)) == (H.state_dim(spec) <= 8)
    elbo, grads = m.elbo_and_grad(data)
    m.dist_p.plan.check_info()
    n1, n2 = host(m.nat1), host(m.nat2)
    want_elbo, want = ref.elbo(n1, n2), ref.gradient(n1, n2)
    e_err, g_err = abs(float(elbo) - want_elbo) / abs(want_elbo), rel(flat(grads), want)
    print(f"{name}-{lik}: elbo {e_err:.2e}, gradient {g_err:.2e} (bound {tol:.0e}); gradient {want}")
    assert e_err <= ELBO_TOL
    assert g_err <= tol
    like = m.kernel.hyperparameter_leaves()
    assert [tuple(g.shape) for g in hyper.flatten(grads)] == [tuple(l.shape) for l in hyper.flatten(like)]
    assert all(g.device.type == "cpu" and str(g.dtype) == "torch.float64" for g in hyper.flatten(grads))


def test_bernoulli_against_difference_quotients(amd, rng):
    """Bernoulli labels: central differences of the model's own classic_elbo with the kernel rebuilt at leaf (1 +- 1e-5) and
    kernel_changed(), the sites untouched; 1e-6 relative to max(1, |g|), the quotient's accuracy."""
    from vidp_amd import hyper, kernels as K
    from vidp_amd.likelihoods import Bernoulli
    from vidp_amd.sparse_variational_cvi import SparseCVIGaussianProcess
    spec = TREES["sum_m52_m32"][0]
    z, t, y = S.make_problem(rng, spec, M_M, N_M, "gaussian")
    lab = (y > 0).astype(np.float64)
    m = SparseCVIGaussianProcess(H.build_vidp(spec), dev(z), Bernoulli(1e-3), learning_rate=0.5)
    data = (dev(t), dev(lab[:, None]))
    for _ in range(2):
        m.update_sites(data)
    _, grads = m.elbo_and_grad(data)
    got = flat(grads)
    like = m.kernel.hyperparameter_values()
    base = [float(v) for v in hyper.flatten(like)]
    fd = []
    for i, v in enumerate(base):
        vals = []
        for s in (+1.0, -1.0):
            x = list(base)
            x[i] = v * (1.0 + s * 1e-5)
            m.kernel.assign_hyperparameters(hyper.unflatten(like, x))
            m.kernel_changed()
            vals.append(float(m.classic_elbo(data)))
        fd.append((vals[0] - vals[1]) / (2e-5 * v))
    m.kernel.assign_hyperparameters(hyper.unflatten(like, list(base)))
    m.kernel_changed()
    err = rel(got, np.array(fd))
    print(f"bernoulli: gradient against difference quotients {err:.2e}; gradient {got}")
    assert err <= 1e-6


# ---- 3. the torch route ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree", ["matern32", "prod_m32_h"])
def test_torch_route_equals_native(amd, rng, monkeypatch, tree):
    """VIDP_NATIVE_SPARSE_SCORE=0 (autograd through kernel._parts, score_fallback) against the HIP route on the same model: the
    kernel bound 5e-12, relative to max(1, |g|)."""
    from vidp_amd import hyper
    spec, jitter = TREES[tree]
    m, data, _ = _model(amd, rng, spec, jitter, "poisson")
    assert hyper.sparse_native_route(m, m._data(data))
    e1, native = m.elbo_and_grad(data)
    monkeypatch.setenv("VIDP_NATIVE_SPARSE_SCORE", "0")
    assert not hyper.sparse_native_route(m, m._data(data))
    e2, torch_route = m.elbo_and_grad(data)
    err = rel(flat(torch_route), flat(native))
    print(f"{tree}: torch route against native {err:.2e}")
    assert float(e1) == float(e2)
    assert err <= KERNEL_TOL


# ---- 4. the fixed point -----------------------------------------------------------------------------------------------------------------------
def test_fisher_term_vanishes_at_the_fixed_point(amd, rng):
    """Gaussian likelihood, lr = 1: the CVI target does not depend on q, so the sites are at their fixed point after one update (three
    are taken); there g^ = theta_s, the chain part's Fisher term is below 1e-10 of the gradient's norm, and the gradient still meets the
    bound of test 2."""
    from vidp_amd import hyper
    spec, jitter = TREES["sum_m52_m32"]
    m, data, ref = _model(amd, rng, spec, jitter, "gaussian", lr=1.0, steps=3)
    parts = {}
    grads = hyper.sparse_elbo_grad(m, data, parts)
    g = flat(grads)
    share = float(np.linalg.norm(flat(parts["chain_fisher"])) / np.linalg.norm(g))
    want = ref.gradient(host(m.nat1), host(m.nat2))
    print(f"fixed point: Fisher share {share:.2e}, gradient {rel(g, want):.2e}")
    assert share < 1e-10
    assert rel(g, want) <= GRAD_TOL
    np.testing.assert_allclose(flat(parts["chain_kl"]) + flat(parts["chain_fisher"]) + flat(parts["conditional"]), g, rtol=1e-13, atol=1e-13)


# ---- 5. out of scope ----------------------------------------------------------------------------------------------------------------------------
def test_out_of_scope_raises(amd, rng):
    """shard=, the three subclasses and a PiecewiseKernel raise NotImplementedError from elbo_and_grad."""
    import torch
    from vidp_amd import kernels as K, space_kernels as SK
    from vidp_amd.likelihoods import Gaussian, HeteroskedasticGaussian, PEPScalarLikelihood
    from vidp_amd.multi_latent_variational import MultiLatentSparseCVI
    from vidp_amd.sparse_pep import SparsePowerExpectationPropagation
    from vidp_amd.sparse_variational_cvi import SparseCVIGaussianProcess
    from vidp_amd.spatio_temporal_variational import SpatioTemporalSparseCVI
    z = dev(np.linspace(0.0, 5.0, 8))
    data = (dev(np.linspace(0.1, 4.9, 10)), dev(rng.normal(size=(10, 1))))
    models = [
        SparsePowerExpectationPropagation(K.Matern32(1.0, 1.0), z, PEPScalarLikelihood(Gaussian(1.0)), learning_rate=0.5, alpha=0.5),
        SpatioTemporalSparseCVI(dev(rng.normal(size=(3, 2))), z, SK.Matern32([0.9, 1.2], 1.0), K.Matern32(1.0, 1.0), Gaussian(1.0)),
        MultiLatentSparseCVI(K.IndependentMultiOutput([K.Matern52(1.0, 1.0), K.Matern32(0.8, 0.5)]), z, HeteroskedasticGaussian()),
        SparseCVIGaussianProcess(K.PiecewiseKernel([K.Matern32(1.0, 1.0), K.Matern32(2.0, 1.0)], torch.tensor([2.5], dtype=torch.float64)),
                                 z, Gaussian(1.0)),
        SparseCVIGaussianProcess(H.build_vidp(SUM9), dev(np.linspace(0.0, 100.0, 200)), Gaussian(1.0),
                                 shard=dict(rank=0, world=2, allreduce=lambda x: x, allgather=lambda x: x[None])),
    ]
    for m in models:
        with pytest.raises(NotImplementedError):
            m.elbo_and_grad(data)


# ---- 6. cache invalidation -------------------------------------------------------------------------------------------------------------------------
def test_kernel_changed_equals_a_fresh_model(amd, rng):
    """assign_hyperparameters + kernel_changed() gives the bound of a freshly built model with the same sites, at 1e-12; without
    kernel_changed() the stale prior answers."""
    from vidp_amd import hyper
    from vidp_amd.likelihoods import Poisson
    from vidp_amd.sparse_variational_cvi import SparseCVIGaussianProcess
    spec, jitter = TREES["sum_m52_m32"]
    m, data, _ = _model(amd, rng, spec, jitter, "poisson")
    before = float(m.classic_elbo(data))
    like = m.kernel.hyperparameter_values()
    new = [1.3 * float(v) for v in hyper.flatten(like)]
    m.kernel.assign_hyperparameters(hyper.unflatten(like, list(new)))
    m.kernel_changed()
    got = float(m.classic_elbo(data))
    fresh = SparseCVIGaussianProcess(H.build_vidp(H.with_params(spec, list(new)), jitter), m.inducing_inputs, Poisson(LIK["poisson"][1]),
                                     learning_rate=0.5)
    fresh.nat1, fresh.nat2 = m.nat1.clone(), m.nat2.clone()
    want = float(fresh.classic_elbo(data))
    assert abs(got - want) <= 1e-12 * abs(want)
    assert abs(got - before) > 1e-3 * abs(before)
    g1, g2 = flat(m.elbo_and_grad(data)[1]), flat(fresh.elbo_and_grad(data)[1])
    assert rel(g1, g2) <= 1e-12


# ---- 7. the trainer ----------------------------------------------------------------------------------------------------------------------------------
def test_trainer_raises_the_elbo(amd):
    """N = 200, M = 25, Bernoulli labels of a Matern-3/2 sample, the lengthscale started at 3 l: fit(20, site_updates=2) raises the
    ELBO, moves the hyper-parameters, and two runs give the identical history."""
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Bernoulli
    from vidp_amd.sparse_variational_cvi import SparseCVIGaussianProcess
    from vidp_amd.trainers import KernelHyperTrainer
    rng = np.random.default_rng(7)
    l, N, M = 1.0, 200, 25
    t = np.sort(rng.uniform(0.0, 20.0, N))
    r = np.abs(t[:, None] - t[None, :])
    Kd = 2.0 * (1.0 + np.sqrt(3.0) * r / l) * np.exp(-np.sqrt(3.0) * r / l)
    f = np.linalg.cholesky(Kd + 1e-9 * np.eye(N)) @ rng.normal(size=N)
    y = (f + 0.3 * rng.normal(size=N) > 0).astype(np.float64)
    z = np.linspace(-0.3, 20.3, M)

    def run():
        m = SparseCVIGaussianProcess(K.Matern32(3.0 * l, 2.0), dev(z), Bernoulli(1e-3), learning_rate=0.5)
        tr = KernelHyperTrainer(m, lr=0.05, input_data=(dev(t), dev(y[:, None])))
        losses = tr.fit(20, site_updates=2)
        return losses, tr.history, m.kernel.hyperparameter_values()
    l1, h1, v1 = run()
    l2, h2, v2 = run()
    print(f"trainer: loss {l1[0]:.4f} -> {l1[-1]:.4f}, hyper-parameters {v1}")
    assert l1[-1] < l1[0]
    assert abs(v1["lengthscale"] - 3.0 * l) > 0.1
    assert l1 == l2 and v1 == v2
    assert [h["hyperparameters"] for h in h1] == [h["hyperparameters"] for h in h2]
