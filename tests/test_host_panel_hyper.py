"""
CPU tests of the panel's hyper-parameter gradient: the restatement tests/np_panel_hyper.py (the sum of B
single-chain restatements of tests/np_sparse_hyper.py, absent points dropped row by row) against central differences of the summed
dense np.longdouble ELBOs, the argument checks and the workspace size of mfgm_panel_cond_score, and that a model on CPU tensors still
refuses.  No GPU.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import np_hyper as H
from tests import np_panel_hyper as PH
from tests import np_sparse_hyper as S

B, M, N = 3, 5, 12
TREES = {name: (spec, jitter) for name, spec, jitter in H.TREES}
LIK = {"gaussian": ("gaussian", 0.3), "poisson": ("poisson", 0.7)}
BOUND = 1e-8          # the bound of tests/test_host_sparse_hyper.py for the same comparison, reasoned there


@pytest.mark.parametrize("tree,lik", [("sum_m52_m32", "gaussian"), ("sum_m52_m32", "poisson")])
def test_restatement_against_finite_differences(rng, tree, lik):
    """sum_b SparseChain.gradient against central differences of sum_b SparseChain.elbo in np.longdouble, B = 3, M = 5, 12 points per
    row, about 15 % of them absent, sites after two damped steps: 1e-8 relative to max(1, |g|).  Measured: 3.3e-12 (Gaussian),
    4.1e-12 (Poisson)."""
    spec, jitter = TREES[tree]
    z, t, y = PH.panel_problem(rng, spec, B, M, N, lik)
    assert 2 <= np.isnan(y).sum() <= 12
    model = PH.Panel(spec, jitter, z, t, y, LIK[lik])
    n1, n2 = model.zero_sites()
    for _ in range(2):
        n1, n2 = model.update_sites(n1, n2, 0.5)
    parts = {}
    got = model.gradient(n1, n2, parts)
    ref = PH.fd_gradient(spec, jitter, z, t, y, LIK[lik], n1, n2).astype(np.float64)
    err = float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))
    print(f"{tree}-{lik}: panel restatement against finite differences {err:.2e}; gradient {ref}")
    assert err <= BOUND
    np.testing.assert_allclose(parts["chain_kl"] + parts["chain_fisher"] + parts["conditional"], got, rtol=1e-12, atol=1e-12)


def test_per_point_conditional_score_sums_to_the_chains(rng):
    """np_panel_hyper.conditional_score on the natural marginals of every series is the conditional part of Panel.gradient."""
    spec, jitter = TREES["matern32"]
    z, t, y = PH.panel_problem(rng, spec, 2, M, 8, "gaussian", absent=0.0)
    model = PH.Panel(spec, jitter, z, t, y, LIK["gaussian"])
    n1, n2 = model.update_sites(*model.zero_sites(), 0.5)
    parts = {}
    model.gradient(n1, n2, parts)
    d = H.state_dim(spec)
    a, b, w, mu, Sig, Sub = [], [], [], [], [], []
    for s, s1, s2 in zip(model.series, n1, n2):
        _, _, av, bv, (m, Sg, _, _) = s.cvi_target(s1, s2)
        blk = lambda i, j: Sg[i * d:(i + 1) * d, j * d:(j + 1) * d]
        a.append(av), b.append(bv), w.append(s.w), mu.append(m.reshape(M, d))
        Sig.append(np.stack([blk(k, k) for k in range(M)]))
        Sub.append(np.stack([blk(k + 1, k) for k in range(M - 1)] + [np.zeros((d, d))]))
    per = PH.conditional_score(spec, jitter, z, t, np.stack(a), np.stack(b), np.stack(w), np.stack(mu), np.stack(Sig), np.stack(Sub),
                               model.series[0].P0)
    got = H.leaves_from_score(spec, per.sum((0, 1)).astype(np.float64))
    np.testing.assert_allclose(got, parts["conditional"], rtol=1e-11, atol=1e-12)


def _plan(lib, B, T, d):
    h = ctypes.c_void_p()
    assert lib.mfgm_plan_create(B, T, d, 0, 0, ctypes.byref(h)) == 0
    return h


def test_panel_cond_score_argument_checks():
    """mfgm_panel_cond_score returns 1 before any HIP call: every null pointer while B N > 0, d = 9, a wide plan, a plan of another
    shape, terms that mfgm_packed_kernel_ssm rejects or whose dimension is not the data's."""
    from vidp_amd import _lib, kernels as K
    lib = _lib.load()
    p = ctypes.c_void_p(8)        # never dereferenced: every call below is refused first
    k = K.Sum([K.Matern32(1.0, 1.0), K.Matern12(1.0, 1.0)])
    kt = k._terms_struct()

    def data(B=3, M=5, d=3, N=7, **holes):
        sd = _lib.PanelData()
        sd.B, sd.M, sd.d, sd.N = B, M, d, N
        sd.idx = sd.seg = sd.w = sd.c = sd.prior_mean = sd.prior_cov = 8
        for name in holes:
            setattr(sd, name, None)
        return sd

    def call(plan, sd, terms, *args):
        return lib.mfgm_panel_cond_score(plan, None if sd is None else ctypes.byref(sd), None if terms is None else ctypes.byref(terms),
                                         *args, None)
    ok_plan, ok = _plan(lib, 3, 5, 3), data()
    assert call(None, ok, kt, *([p] * 10)) == 1
    assert call(ok_plan, None, kt, *([p] * 10)) == 1
    assert call(ok_plan, ok, None, *([p] * 10)) == 1
    for hole in range(10):          # gap_lo, gap_hi, a, b, x, Sig, Sub, score, ws, info
        args = [p] * 10
        args[hole] = None
        assert call(ok_plan, ok, kt, *args) == 1, hole
    for field in ("idx", "w", "prior_mean", "prior_cov"):
        assert call(ok_plan, data(**{field: None}), kt, *([p] * 10)) == 1, field
    assert call(_plan(lib, 3, 5, 9), data(d=9), kt, *([p] * 10)) == 1                            # d = 9 (and its plan is wide)
    assert call(_plan(lib, 3, 5, 9), ok, kt, *([p] * 10)) == 1                                   # a wide plan
    for other in (_plan(lib, 2, 5, 3), _plan(lib, 3, 6, 3), _plan(lib, 3, 5, 2)):
        assert call(other, ok, kt, *([p] * 10)) == 1                                             # the plan is not the data's
    assert call(_plan(lib, 3, 5, 2), data(d=2), kt, *([p] * 10)) == 1                            # not the tree's dimension
    bad = k._terms_struct()
    bad.kind[0][0] = 9
    assert call(ok_plan, ok, bad, *([p] * 10)) == 1
    bad = k._terms_struct()
    bad.offset[1] = 1
    assert call(ok_plan, ok, bad, *([p] * 10)) == 1


def test_panel_cond_score_workspace():
    """One partial per wavefront of 64 points and plane: positive at B N = 1, monotone in B N."""
    from vidp_amd import _lib
    lib = _lib.load()
    size = lib.mfgm_panel_cond_score_workspace_doubles
    assert size(1, 1) == 48 and size(3, 70) == 48 * 4 and size(0, 5) == 48 and size(4096, 512) == 48 * 32768
    sizes = [size(b, n) for b, n in ((1, 1), (1, 64), (1, 65), (3, 70), (8, 70), (8, 512), (4096, 512))]
    assert sizes == sorted(sizes) and sizes[0] > 0


def test_cpu_model_refuses_and_overlap_add_takes_a_batch(rng):
    """elbo_and_grad on CPU tensors raises before the data is looked at; hyper.overlap_add with a leading series axis is the
    single-chain overlap-add row by row; kernel_changed() drops the caches and keeps the sites."""
    import vidp_amd
    from vidp_amd import hyper, kernels as K
    from vidp_amd.likelihoods import Gaussian
    z = torch.linspace(0.0, 2.0, 6, dtype=torch.float64)
    m = vidp_amd.PanelSparseCVI(K.Matern32(1.0, 1.0), z, Gaussian(0.1), 3)
    with pytest.raises(NotImplementedError, match="out of scope"):
        m.elbo_and_grad(None)
    n1, n2 = torch.from_numpy(rng.normal(size=(3, 7, 4))), torch.from_numpy(rng.normal(size=(3, 7, 4, 4)))
    got = hyper.overlap_add(n1, n2)
    for b in range(3):
        for x, y in zip(got, hyper.overlap_add(n1[b], n2[b])):
            assert torch.equal(x[b], y)
    t = torch.sort(torch.from_numpy(rng.uniform(0.0, 2.0, size=(3, 9))), dim=1).values
    data = (t, torch.from_numpy(rng.normal(size=(3, 9, 1))))
    m.update_sites(data)
    before, sites = float(m.classic_elbo(data)), m.nat1.clone()
    m.kernel.assign_hyperparameters(dict(lengthscale=2.0, variance=1.0))
    assert float(m.classic_elbo(data)) == before          # the stale prior answers
    m.kernel_changed()
    assert abs(float(m.classic_elbo(data)) - before) > 1e-6 * abs(before)
    assert torch.equal(m.nat1, sites)
    fresh = vidp_amd.PanelSparseCVI(K.Matern32(2.0, 1.0), z, Gaussian(0.1), 3)
    fresh.nat1, fresh.nat2 = m.nat1.clone(), m.nat2.clone()
    assert float(fresh.classic_elbo(data)) == float(m.classic_elbo(data))
