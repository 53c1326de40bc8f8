"""
GPU tests of the panel's hyper-parameter gradient: k_panel_cond_score (csrc/mfgm_panel_score.h, entry point
mfgm_panel_cond_score) against the np.longdouble restatement on identical inputs for every block size and two partitions of the
plan, PanelSparseCVI.elbo_and_grad against the restatement tests/np_panel_hyper.py (the sum of B single-chain restatements), against
the sum of B single-chain models and against difference quotients of the model's own bound, the torch route, the fixed point,
kernel_changed(), KernelHyperTrainer and what is refused.  fp64.

Measured on an MI355X: kernel against long double worst 9.4e-15 of the absolute sum (bound 5e-12); elbo_and_grad against the
restatement 3.9e-16 (bound) and 8.2e-15 (gradients), against B single-chain models 0 and 2.1e-15 (bounds 1e-9 / 1e-8); Bernoulli
against difference quotients 1.9e-9 (bound 1e-6); torch route against the HIP route 7.8e-16 (bound 5e-12); Fisher share at the
Gaussian fixed point 1.1e-17 (bound 1e-9).
"""
import ctypes

import numpy as np
import pytest

from tests import np_hyper as H
from tests import np_panel_hyper as PH
from tests import np_sparse_hyper as S
from tests.test_gpu_sparse_hyper import ELBO_TOL, GRAD_TOL, KERNEL_CASES, KERNEL_TOL, TREES, _pair_chain, dev, flat, host, rel

pytestmark = pytest.mark.gpu

LIK = {"gaussian": ("gaussian", 0.3), "poisson": ("poisson", 0.7), "bernoulli": ("bernoulli", 1e-3)}
SUM8 = "sum_m52_m52_m32"          # 3 + 3 + 2


@pytest.fixture(scope="module")
def amd():
    import torch
    import vidp_amd
    assert torch.cuda.is_available()
    vidp_amd._lib.load()
    return vidp_amd


def _likelihood(kind):
    from vidp_amd.likelihoods import Bernoulli, Gaussian, Poisson
    return {"gaussian": Gaussian, "poisson": Poisson, "bernoulli": Bernoulli}[kind](LIK[kind][1])


# ---- 1. the kernel alone ------------------------------------------------------------------------------------------------------------------
B_K, M_K = 3, 5


def _row_times(rng, z, lm, N, b):
    """N sorted points of one row: both end intervals hold points, interval 2 is empty, two points share one time, one point sits
    exactly on an inducing point; every other gap is at least half the tree's shortest time scale."""
    if N == 1:
        return np.array([z[b + 1] + 0.7 * lm])
    cells = np.concatenate([[z[0] - 2.0 * lm], z, [z[-1] + 2.0 * lm]])
    k = rng.choice([0, 1, 3, 4, 5], N - 2)
    k[:4] = (0, 0, 5, 5)
    lo, hi = cells[k] + 0.5 * lm, cells[k + 1] - 0.5 * lm
    t = lo + rng.uniform(0, 1, N - 2) * (hi - lo)
    return np.sort(np.concatenate([t, [t[7]], [z[3]]]))


def _panel_struct(amd, B, d, N, keep):
    sd = amd._lib.PanelData()
    sd.B, sd.M, sd.d, sd.N = B, M_K, d, N
    sd.idx, sd.w, sd.c, sd.prior_mean, sd.prior_cov = (x.data_ptr() for x in keep)
    sd.seg = None          # not read
    return sd


@pytest.mark.parametrize("N", [1, 70])
@pytest.mark.parametrize("tree,jitter", KERNEL_CASES, ids=[f"{t}-{j:g}" for t, j in KERNEL_CASES])
def test_panel_cond_score_kernel_against_long_double(amd, rng, tree, jitter, N):
    """mfgm_panel_cond_score through the C ABI against the np.longdouble restatement on identical inputs: B = 3, M = 5, N = 1 and 70
    (B N = 210 is no multiple of 64: series boundaries fall inside a wavefront), a = b = 0 on about 15 % of the points and on the whole
    last series, random positive definite pair moments per series packed with Plan.pack, on the default partition and on
    Plan(3, 5, d, R0=2), whose pairs (m - 1, m) straddle segment boundaries.  Bound: 5e-12 of the sum of the absolute per-point
    contributions to the slot; absent slots exactly zero; identical bits on a second call and on the two partitions; the same bits
    without the all-zero series; *info == 0."""
    import torch
    spec = TREES[tree][0]
    d = H.state_dim(spec)
    lm = H.shortest_lengthscale(spec)
    z = np.cumsum(rng.uniform(2.0, 3.0, M_K) * lm)
    t = np.stack([_row_times(rng, z, lm, N, b) for b in range(B_K)])
    idx, glo, ghi = (np.stack(x) for x in zip(*[S.gaps(tb, z) for tb in t]))
    if N > 1:
        for b in range(B_K):
            assert (idx[b] == 0).sum() >= 2 and (idx[b] == M_K).sum() >= 2 and (idx[b] == 2).sum() == 0 and (ghi[b] == 0.0).sum() == 1
            assert (np.diff(t[b]) == 0.0).sum() == 1
    w = np.stack([S.conditional_stats(spec, jitter, glo[b], ghi[b], np.float64)[0] for b in range(B_K)])
    a, b = rng.normal(size=(B_K, N)), -rng.uniform(0.1, 1.0, (B_K, N))
    gone = rng.uniform(size=(B_K, N)) < 0.15
    gone[-1] = True                                  # a series without observations
    if N > 1:
        gone[0, 0] = False
        assert 0.05 * 2 * N < gone[:2].sum() < 0.3 * 2 * N
    a[gone], b[gone] = 0.0, 0.0
    mu, Sig, Sub = (np.stack(x) for x in zip(*[_pair_chain(rng, M_K, d) for _ in range(B_K)]))
    P0 = S.transition(spec, jitter, 0.0, np.float64)[2] + jitter * np.eye(d)
    per = PH.conditional_score(spec, jitter, z, t, a, b, w, mu, Sig, Sub, P0)
    assert (per[-1] == 0.0).all() and (per[gone] == 0.0).all()
    ref, scale = per.sum((0, 1)).astype(np.float64), np.abs(per).sum((0, 1)).astype(np.float64)
    # the device
    lib = amd._lib.load()
    kt = H.build_vidp(spec, jitter)._terms_struct()

    def run(B, plan):
        keep = [dev(idx[:B], np.int32), dev(w[:B]), dev(np.zeros((B, N))), dev(np.zeros(d)), dev(P0)]
        sd = _panel_struct(amd, B, d, N, keep)
        args = [dev(glo[:B]), dev(ghi[:B]), dev(a[:B]), dev(b[:B]), plan.pack(amd.VEC, dev(mu[:B])), plan.pack(amd.SYM, dev(Sig[:B])),
                plan.pack(amd.FULL, dev(Sub[:B, :M_K - 1]))]
        ws = torch.empty(int(lib.mfgm_panel_cond_score_workspace_doubles(B, N)), dtype=torch.float64, device="cuda")
        out = []
        for _ in range(2):
            score = torch.full((8, 3, 2), np.nan, dtype=torch.float64, device="cuda")
            rc = lib.mfgm_panel_cond_score(plan.h, ctypes.byref(sd), ctypes.byref(kt), *[x.data_ptr() for x in args], score.data_ptr(),
                                           ws.data_ptr(), plan.info.data_ptr(), None)
            assert rc == 0
            out.append(score)
        torch.cuda.synchronize()
        assert int(plan.info.item()) == 0
        assert torch.equal(out[0], out[1])
        return host(out[0])

    g = run(B_K, amd.Plan(B_K, M_K, d))
    split = amd.Plan(B_K, M_K, d, R0=2)
    assert split.P > 1
    assert np.array_equal(run(B_K, split), g)                              # the partition moves the addresses, not the sums
    assert np.array_equal(run(B_K - 1, amd.Plan(B_K - 1, M_K, d)), g)      # the all-zero series adds exact zeros
    nt = ref.shape[0]
    present = np.zeros((8, 3, 2), dtype=bool)
    for ci, term in enumerate(H.terms_of(spec)):
        for f, leaf in enumerate(term):
            present[ci, f] = True
    assert (g[~present] == 0.0).all()
    err = np.abs(g[:nt] - ref)[present[:nt]] / np.maximum(scale, 1e-300)[present[:nt]]
    err = err[scale[present[:nt]] > 0]
    print(f"{tree} jitter {jitter} N {N}: panel kernel against long double {err.max():.2e} of the absolute sum (bound {KERNEL_TOL:.0e})")
    assert err.max() <= KERNEL_TOL


def test_panel_cond_score_without_points(amd):
    """B N = 0 writes a zero score and returns 0 with no array but the score."""
    import torch
    lib = amd._lib.load()
    spec, jitter = TREES["sum_m52_m32"]
    d = H.state_dim(spec)
    plan = amd.Plan(B_K, M_K, d)
    sd = amd._lib.PanelData()
    sd.B, sd.M, sd.d, sd.N = B_K, M_K, d, 0
    kt = H.build_vidp(spec, jitter)._terms_struct()
    score = torch.full((8, 3, 2), np.nan, dtype=torch.float64, device="cuda")
    assert lib.mfgm_panel_cond_score(plan.h, ctypes.byref(sd), ctypes.byref(kt), *([None] * 7), score.data_ptr(), None, None, None) == 0
    assert (host(score) == 0.0).all()


# ---- 2. the model ---------------------------------------------------------------------------------------------------------------------------
B_M, M_M, N_M = 4, 6, 40
MODEL_CASES = [("matern32", "gaussian"), ("matern52", "poisson"), (SUM8, "bernoulli")]


def _model(amd, rng, tree, lik, lr=0.5, steps=2, B=B_M, M=M_M, N=N_M):
    """(model, data, (spec, jitter, z, t, y)) after `steps` update_sites at learning rate lr; ragged rows (NaN observations)."""
    spec, jitter = TREES[tree]
    z, t, y = PH.panel_problem(rng, spec, B, M, N, lik)
    assert np.isnan(y).sum() > 0.05 * B * N
    m = amd.PanelSparseCVI(H.build_vidp(spec, jitter), dev(z), _likelihood(lik), B, learning_rate=lr)
    data = (dev(t), dev(y[..., None]))
    for _ in range(steps):
        m.update_sites(data)
    return m, data, (spec, jitter, z, t, y)


@pytest.mark.parametrize("tree,lik", MODEL_CASES, ids=[f"{a}-{b}" for a, b in MODEL_CASES])
def test_elbo_and_grad_against_restatement_and_single_chains(amd, rng, tree, lik):
    """elbo_and_grad after two update_sites at lr = 0.5, B = 4, M = 6, N = 40, about 15 % of the observations NaN, against (i) the
    restatement at the model's own sites and (ii) the sum of B SparseCVIGaussianProcess.elbo_and_grad with the series' sites assigned
    and its absent points removed: the bound at 1e-9 relative, the gradients at 1e-8 relative to max(1, |g|)."""
    from vidp_amd import hyper
    from vidp_amd.sparse_variational_cvi import SparseCVIGaussianProcess
    m, data, (spec, jitter, z, t, y) = _model(amd, rng, tree, lik)
    assert hyper.panel_native_route(m)
    elbo, grads = m.elbo_and_grad(data)
    m.dist_p.plan.check_info()
    got = flat(grads)
    like = m.kernel.hyperparameter_leaves()
    assert [tuple(g.shape) for g in hyper.flatten(grads)] == [tuple(l.shape) for l in hyper.flatten(like)]
    assert all(g.device.type == "cpu" and str(g.dtype) == "torch.float64" for g in hyper.flatten(grads))
    n1, n2 = host(m.nat1), host(m.nat2)
    ref = PH.Panel(spec, jitter, z, t, y, LIK[lik])
    want_elbo, want = ref.elbo(n1, n2), ref.gradient(n1, n2)
    e_err, g_err = abs(float(elbo) - want_elbo) / abs(want_elbo), rel(got, want)
    print(f"{tree}-{lik}: against the restatement: elbo {e_err:.2e} (bound {ELBO_TOL:.0e}), gradient {g_err:.2e} (bound {GRAD_TOL:.0e}); "
          f"gradient {want}")
    s_elbo, s_grad = 0.0, 0.0
    for b, (tb, yb) in enumerate(PH.present(t, y)):
        one = SparseCVIGaussianProcess(H.build_vidp(spec, jitter), dev(z), _likelihood(lik), learning_rate=0.5)
        one.nat1, one.nat2 = m.nat1[b].clone(), m.nat2[b].clone()
        e, g = one.elbo_and_grad((dev(tb), dev(yb[:, None])))
        s_elbo, s_grad = s_elbo + float(e), s_grad + flat(g)
    e2, g2 = abs(float(elbo) - s_elbo) / abs(s_elbo), rel(got, s_grad)
    print(f"{tree}-{lik}: against {B_M} single-chain models: elbo {e2:.2e}, gradient {g2:.2e}")
    assert e_err <= ELBO_TOL and e2 <= ELBO_TOL
    assert g_err <= GRAD_TOL and g2 <= GRAD_TOL


# ---- 3. difference quotients of the model's own bound ----------------------------------------------------------------------------------------
def test_bernoulli_against_difference_quotients(amd, rng):
    """Bernoulli labels: central differences of the model's own classic_elbo with the kernel at leaf (1 +- 1e-6) and kernel_changed()
    between the evaluations, the sites untouched; 1e-6 relative to max(1, |g|)."""
    from vidp_amd import hyper
    m, data, _ = _model(amd, rng, "sum_m52_m32", "bernoulli")
    got = flat(m.elbo_and_grad(data)[1])
    like = m.kernel.hyperparameter_values()
    base = [float(v) for v in hyper.flatten(like)]
    fd = []
    for i, v in enumerate(base):
        vals = []
        for s in (+1.0, -1.0):
            x = list(base)
            x[i] = v * (1.0 + s * 1e-6)
            m.kernel.assign_hyperparameters(hyper.unflatten(like, x))
            m.kernel_changed()
            vals.append(float(m.classic_elbo(data)))
        fd.append((vals[0] - vals[1]) / (2e-6 * v))
    m.kernel.assign_hyperparameters(hyper.unflatten(like, list(base)))
    m.kernel_changed()
    err = rel(got, np.array(fd))
    print(f"bernoulli: panel gradient against difference quotients {err:.2e} (bound 1e-06); gradient {got}")
    assert err <= 1e-6


# ---- 4. the torch route ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", ["VIDP_NATIVE_SPARSE_SCORE", "VIDP_NATIVE_PANEL"])
@pytest.mark.parametrize("tree", ["matern32", "prod_m32_h"])
def test_torch_route_equals_native(amd, rng, monkeypatch, tree, switch):
    """VIDP_NATIVE_SPARSE_SCORE=0 and VIDP_NATIVE_PANEL=0 (autograd through kernel._parts on the gathered pair moments,
    score_fallback) against the HIP route on the same model: the kernel bound 5e-12, relative to max(1, |g|)."""
    from vidp_amd import hyper
    m, data, _ = _model(amd, rng, tree, "poisson")
    assert hyper.panel_native_route(m)
    e1, native = m.elbo_and_grad(data)
    monkeypatch.setenv(switch, "0")
    assert not hyper.panel_native_route(m)
    m.nat1 = m.nat1.clone()          # moves the stamp: the torch route makes its own predictions
    e2, torch_route = m.elbo_and_grad(data)
    err = rel(flat(torch_route), flat(native))
    print(f"{tree} {switch}=0: torch route against native {err:.2e} (bound {KERNEL_TOL:.0e})")
    assert abs(float(e1) - float(e2)) <= ELBO_TOL * abs(float(e1))
    assert err <= KERNEL_TOL


def test_leg_against_difference_quotients(amd, rng):
    """The LEG kernel (d = 3, torch route) against central differences of the model's own classic_elbo in entries of N and R with
    kernel_changed() between the evaluations, e = 1e-5: 1e-6 relative, the bound tests/test_gpu_hyper.py uses for the LEG kernel."""
    import torch
    from vidp_amd import hyper, kernels as K
    from vidp_amd.likelihoods import Gaussian
    Nm = torch.tensor([[0.9, 0.2, 0.0], [-0.1, 0.7, 0.3], [0.2, 0.0, 1.1]], dtype=torch.float64)
    Rm = torch.tensor([[0.0, 0.8, -0.3], [0.1, 0.0, 0.5], [0.0, -0.2, 0.0]], dtype=torch.float64)
    z, t, y = PH.panel_problem(rng, H.M32, 3, M_M, 20, "gaussian")
    m = amd.PanelSparseCVI(K.LatentExponentiallyGenerated(Nm, Rm), dev(z), Gaussian(0.3), 3, learning_rate=0.5)
    data = (dev(t), dev(y[..., None]))
    for _ in range(2):
        m.update_sites(data)
    assert not hyper.panel_native_route(m)
    _, grads = m.elbo_and_grad(data)
    for nm, M0 in (("N", Nm), ("R", Rm)):
        for (i, j) in ((0, 0), (1, 2), (2, 1)):
            def at(e):
                Mx = M0.clone()
                Mx[i, j] += e
                m.kernel.assign_hyperparameters({"N": Mx if nm == "N" else Nm, "R": Mx if nm == "R" else Rm})
                m.kernel_changed()
                return float(m.classic_elbo(data))
            fd = (at(1e-5) - at(-1e-5)) / 2e-5
            print(f"LEG {nm}[{i}, {j}]: {float(grads[nm][i, j]):.10e} quotient {fd:.10e}")
            assert abs(float(grads[nm][i, j]) - fd) <= 1e-6 * abs(fd), (nm, i, j)          # (R's diagonal does not act: 0 = 0)
    m.kernel.assign_hyperparameters({"N": Nm, "R": Rm})
    m.kernel_changed()


# ---- 5. the fixed point -----------------------------------------------------------------------------------------------------------------------
def test_fisher_term_vanishes_at_the_fixed_point(amd, rng):
    """Gaussian likelihood: the CVI target does not depend on q, so one update_sites at lr = 1 puts every series at its fixed point;
    there g^ = theta_s and the chain part's Fisher term is below 1e-9 of the gradient's scale, and the parts add up."""
    from vidp_amd import hyper
    m, data, (spec, jitter, z, t, y) = _model(amd, rng, "sum_m52_m32", "gaussian", lr=1.0, steps=1)
    parts = {}
    g = flat(hyper.panel_elbo_grad(m, data, parts))
    share = float(np.linalg.norm(flat(parts["chain_fisher"])) / np.linalg.norm(g))
    want = PH.Panel(spec, jitter, z, t, y, LIK["gaussian"]).gradient(host(m.nat1), host(m.nat2))
    print(f"fixed point: Fisher share {share:.2e} (bound 1e-09), gradient {rel(g, want):.2e}")
    assert share <= 1e-9
    assert rel(g, want) <= GRAD_TOL
    np.testing.assert_allclose(flat(parts["chain_kl"]) + flat(parts["chain_fisher"]) + flat(parts["conditional"]), g, rtol=1e-13, atol=1e-13)


# ---- 6. cache invalidation -------------------------------------------------------------------------------------------------------------------
def test_kernel_changed_equals_a_fresh_model(amd, rng):
    """assign_hyperparameters + kernel_changed() gives the bound and the gradient of a freshly built model with the same sites, to the
    last bit on the native route; without kernel_changed() the stale prior answers."""
    from vidp_amd import hyper
    m, data, (spec, jitter, z, t, y) = _model(amd, rng, "sum_m52_m32", "poisson")
    before = float(m.classic_elbo(data))
    like = m.kernel.hyperparameter_values()
    new = [1.3 * float(v) for v in hyper.flatten(like)]
    m.kernel.assign_hyperparameters(hyper.unflatten(like, list(new)))
    assert float(m.classic_elbo(data)) == before
    m.kernel_changed()
    assert hyper.panel_native_route(m)
    got, grads = m.elbo_and_grad(data)
    fresh = amd.PanelSparseCVI(H.build_vidp(H.with_params(spec, list(new)), jitter), m.inducing_inputs, _likelihood("poisson"), B_M,
                               learning_rate=0.5)
    fresh.nat1, fresh.nat2 = m.nat1.clone(), m.nat2.clone()
    want, wgrads = fresh.elbo_and_grad(data)
    assert float(got) == float(want) == float(m.classic_elbo(data))
    assert abs(float(got) - before) > 1e-3 * abs(before)
    assert np.array_equal(flat(grads), flat(wgrads))


# ---- 7. the trainer ----------------------------------------------------------------------------------------------------------------------------
def test_trainer_raises_the_elbo(amd):
    """B = 8 Gaussian series of N = 60 points drawn from a Matern-3/2 with lengthscale l, M = 16, the model started at l / 4:
    fit(10, site_updates=2) raises the ELBO and moves the lengthscale towards l.  Not a convergence claim."""
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Gaussian
    from vidp_amd.trainers import KernelHyperTrainer
    rng = np.random.default_rng(11)
    l, B, N, M = 2.0, 8, 60, 16
    t = np.sort(rng.uniform(0.0, 12.0, (B, N)), axis=1)
    y = np.zeros((B, N))
    for b in range(B):
        r = np.abs(t[b][:, None] - t[b][None, :])
        Kd = 1.5 * (1.0 + np.sqrt(3.0) * r / l) * np.exp(-np.sqrt(3.0) * r / l)
        y[b] = np.linalg.cholesky(Kd + 1e-9 * np.eye(N)) @ rng.normal(size=N) + 0.3 * rng.normal(size=N)
    z = np.linspace(-0.3, 12.3, M)
    m = amd.PanelSparseCVI(K.Matern32(l / 4.0, 1.5), dev(z), Gaussian(0.09), B, learning_rate=0.5)
    tr = KernelHyperTrainer(m, lr=0.05, input_data=(dev(t), dev(y[..., None])))
    losses = tr.fit(10, site_updates=2)
    v = m.kernel.hyperparameter_values()
    print(f"panel trainer: loss {losses[0]:.4f} -> {losses[-1]:.4f}, hyper-parameters {v}")
    assert losses[-1] < losses[0]
    assert l / 4.0 + 0.05 < v["lengthscale"] < l
    assert len(tr.history) == 10


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(amd, rng):
    """d > 8 raises NotImplementedError naming the state dimension, a PiecewiseKernel is refused, and a noise-free HarmonicOscillator
    term without jitter raises ValueError before anything is built."""
    import torch
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Gaussian
    z = dev(np.linspace(0.0, 5.0, 8))
    data = (dev(np.sort(rng.uniform(0.1, 4.9, (2, 10)), axis=1)), dev(rng.normal(size=(2, 10, 1))))
    nine = amd.PanelSparseCVI(K.Sum([K.Matern52(1.3, 0.8), K.Matern52(0.8, 0.6), K.Matern52(2.1, 1.4)]), z, Gaussian(1.0), 2)
    with pytest.raises(NotImplementedError, match="state dimension 9"):
        nine.elbo_and_grad(data)
    with pytest.raises(NotImplementedError):
        amd.PanelSparseCVI(K.PiecewiseKernel([K.Matern32(1.0, 1.0), K.Matern32(2.0, 1.0)], torch.tensor([2.5], dtype=torch.float64)),
                           z, Gaussian(1.0), 2)
    osc = amd.PanelSparseCVI(K.Sum([K.Matern32(1.0, 1.0), K.HarmonicOscillator(1.0, 2.0)]), z, Gaussian(1.0), 2)
    with pytest.raises(ValueError, match="HarmonicOscillator"):
        osc.elbo_and_grad(data)
    assert osc._dist_p is None          # refused before the prior was built
