"""
CPU tests of the sparse-CVI hyper-parameter gradient: the NumPy restatement of the whole gradient
(tests/np_sparse_hyper.py: chain part on moments displaced by a dense Fisher-vector product, conditional part as
csrc/mfgm_sparse_score.h differentiates it) against central differences of a dense np.longdouble ELBO at fixed sites, the torch
restatement of the conditional part (vidp_amd.hyper.conditional_part_torch) against the NumPy one, the argument checks of
mfgm_sparse_cond_score and of the trainer.  No GPU.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import np_hyper as H
from tests import np_sparse_hyper as S

M, N = 6, 30
TREES = {name: (spec, jitter) for name, spec, jitter in H.TREES}
CASES = [("matern52", "gaussian"), ("matern52", "poisson"), ("sum_m52_m32", "gaussian"), ("sum_m52_m32", "poisson"),
         ("prod_m32_h", "gaussian"), ("prod_m32_h", "poisson")]
LIK = {"gaussian": ("gaussian", 0.3), "poisson": ("poisson", 0.7)}
# The yardstick's own error, relative to max(1, |g|): truncation h^2 |g'''| / 6 with h = 1e-6 |leaf| (1.7e-13 |leaf|^3 |g'''|, and
# |leaf|^3 |g'''| stays below ~1e3 |g| for these kernels) plus rounding eps_longdouble cond(K) |L| / h ~ 1.1e-19 * 1e4 * 1e2 / 1e-6 =
# 1.1e-7 at the very worst conditioning, typically 1e4 x smaller.  The fp64 restatement adds FP64_SPREAD-sized rounding.  Bounded at
# 1e-8, the end-to-end accuracy tests/test_gpu_hyper.py states for the d <= 8 plans; measured values are printed and in DESIGN 21.
BOUND = 1e-8


def _sites(model):
    """Sites after two damped steps (lr = 0.5) of the restatement's own CVI update, from zero."""
    n1, n2 = model.zero_sites()
    for _ in range(2):
        n1, n2 = model.update_sites(n1, n2, 0.5)
    return n1, n2


@pytest.mark.parametrize("tree,lik", CASES, ids=[f"{a}-{b}" for a, b in CASES])
def test_restatement_against_finite_differences(rng, tree, lik):
    """The fp64 restatement of d ELBO / d leaves at fixed sites against the yardstick, M = 6, N = 30, relative to max(1, |g|).
    Measured: matern52 1.8e-12 / 1.7e-12 (Gaussian / Poisson), sum_m52_m32 3.3e-12 / 3.6e-12, prod_m32_h 1.1e-10 / 4.7e-11.
    The F (g^ - theta_s) share of the gradient is asserted to be at least 1e-3 of its norm (measured 6.2e-3 .. 1.3e-2), so a
    gradient without that term misses the bound by more than three orders of magnitude, which is asserted too."""
    spec, jitter = TREES[tree]
    z, t, y = S.make_problem(rng, spec, M, N, lik)
    model = S.SparseChain(spec, jitter, z, t, y, LIK[lik])
    n1, n2 = _sites(model)
    parts = {}
    got = model.gradient(n1, n2, parts)
    ref = S.fd_gradient(spec, jitter, z, t, y, LIK[lik], n1, n2).astype(np.float64)
    err = float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))
    share = float(np.linalg.norm(parts["chain_fisher"]) / np.linalg.norm(ref))
    print(f"{tree}-{lik}: restatement against finite differences {err:.2e}; Fisher share {share:.2e}; gradient {ref}")
    assert share >= 1e-3
    assert err <= BOUND
    without = got - parts["chain_fisher"]
    assert float(np.max(np.abs(without - ref) / np.maximum(1.0, np.abs(ref)))) > 1e3 * BOUND


def test_elbo_restatement_is_the_oracles_at_zero_sites(rng):
    """At zero sites q = p: KL = 0 and the bound is the sum of the variational expectations under the prior marginals k(t, t)."""
    spec, jitter = TREES["sum_m52_m32"]
    z, t, y = S.make_problem(rng, spec, M, N, "gaussian")
    model = S.SparseChain(spec, jitter, z, t, y, LIK["gaussian"])
    n1, n2 = model.zero_sites()
    mu, Sigma = model.posterior(n1, n2)
    fmu, fvar, _, _ = model.predict(mu, Sigma)
    np.testing.assert_allclose(fmu, 0.0, atol=1e-13)
    np.testing.assert_allclose(fvar, H.k_closed(spec, np.zeros(N)), rtol=1e-10)
    ve = S.ve_and_grads(LIK["gaussian"], fmu, fvar, y)[0].sum()
    assert abs(model.elbo(n1, n2) - ve) <= 1e-9 * abs(ve)


@pytest.mark.parametrize("tree", ["matern52", "sum_m52_m32", "prod_m32_h", "sum_prod_m12_h_const"])
def test_torch_conditional_part_is_the_restatement(rng, tree):
    """hyper.conditional_part_torch (autograd through kernel._parts and the three lines of the covariance form) against the NumPy
    reverse mode on random cotangents and positive definite pair moments, on the CPU; points in both end intervals and one on an
    inducing point."""
    from vidp_amd import hyper
    spec, jitter = TREES[tree]
    d = H.state_dim(spec)
    z, t, _ = S.make_problem(rng, spec, M, 12, "gaussian")
    t[5] = z[2]
    t = np.sort(t)
    idx, glo, ghi = S.gaps(t, z)
    n = len(t)
    a, b = rng.normal(size=n), -np.abs(rng.normal(size=n))
    w, _ = S.conditional_stats(spec, jitter, glo, ghi, np.float64)
    L = rng.normal(size=(n, 2 * d, 2 * d))
    Sp = L @ L.transpose(0, 2, 1) + 0.5 * np.eye(2 * d)
    P0 = S.transition(spec, jitter, 0.0, np.float64)[2] + jitter * np.eye(d)
    Sp[idx == 0, :d, :d] = P0
    Sp[idx == M, d:, d:] = P0
    mp = rng.normal(size=(n, 2 * d))
    wbar = a[:, None] * mp + 2.0 * b[:, None] * np.einsum("ijk,ik->ij", Sp, w)
    ref = H.leaves_from_score(spec, S.conditional_score(spec, jitter, glo, ghi, idx, M, a, b, wbar, w).sum(0))
    k = H.build_vidp(spec, jitter)
    tt = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    got = hyper.conditional_part_torch(k, tt(glo), tt(ghi), tt(a), tt(b), tt(mp), tt(Sp), tt(idx), M)
    got = np.array([float(g) for g in hyper.flatten(got)])
    err = float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))
    print(f"{tree}: torch conditional part against the restatement {err:.2e}")
    assert err <= 1e-10


def test_overlap_add_is_the_dense_assembly(rng):
    """hyper.overlap_add lays pair sites out on the chain as mfgm_sparse_theta does: the same quadratic form as the dense assembly."""
    from vidp_amd import hyper
    spec, jitter = TREES["matern32"]
    z, t, y = S.make_problem(rng, spec, 4, 6, "gaussian")
    model = S.SparseChain(spec, jitter, z, t, y, LIK["gaussian"])
    d, m = model.d, model.M
    n1 = rng.normal(size=(m + 1, 2 * d))
    n2 = rng.normal(size=(m + 1, 2 * d, 2 * d))
    n2 = n2 + n2.transpose(0, 2, 1)
    v, V = model.dense_naturals(n1, n2)
    lin, diag, sub = (x.numpy() for x in hyper.overlap_add(torch.from_numpy(n1), torch.from_numpy(n2)))
    s = rng.normal(size=(m, d))
    dense = v @ s.reshape(-1) + s.reshape(-1) @ V @ s.reshape(-1)
    chain = (lin * s).sum() + np.einsum("ti,tij,tj->", s, diag, s) + np.einsum("ti,tij,tj->", s[1:], sub, s[:-1])
    assert abs(dense - chain) <= 1e-12 * max(1.0, abs(dense))


def test_cond_score_argument_checks():
    """mfgm_sparse_cond_score returns 1 before any HIP call: null pointers, d > 8, a sharded data set, terms that
    mfgm_packed_kernel_ssm rejects, a tree whose dimension is not the data's."""
    from vidp_amd import _lib, kernels as K
    lib = _lib.load()
    p = ctypes.c_void_p(8)        # never dereferenced: every call below is refused first
    k = K.Sum([K.Matern32(1.0, 1.0), K.Matern12(1.0, 1.0)])
    kt = k._terms_struct()

    def data(d=3, m_hi=0):
        sd = _lib.SparseData()
        sd.M, sd.d, sd.N, sd.m_lo, sd.m_hi = 5, d, 7, 0, m_hi
        sd.seg = sd.w = sd.c = sd.prior_mean = sd.prior_cov = 8
        return sd
    call = lambda sd, terms, *a: lib.mfgm_sparse_cond_score(None if sd is None else ctypes.byref(sd), terms, *a)
    ok = data()
    assert call(None, ctypes.byref(kt), *([p] * 10), None) == 1
    assert call(ok, None, *([p] * 10), None) == 1
    for hole in range(10):
        args = [p] * 10
        args[hole] = None
        assert call(ok, ctypes.byref(kt), *args, None) == 1, hole
    for field in ("seg", "w", "prior_mean", "prior_cov"):
        sd = data()
        setattr(sd, field, None)
        assert call(sd, ctypes.byref(kt), *([p] * 10), None) == 1, field
    assert call(data(d=9), ctypes.byref(kt), *([p] * 10), None) == 1          # d > 8
    assert call(data(d=2), ctypes.byref(kt), *([p] * 10), None) == 1          # not the tree's dimension
    assert call(data(m_hi=3), ctypes.byref(kt), *([p] * 10), None) == 1       # a chain shared between processes
    bad = k._terms_struct()
    bad.kind[0][0] = 9
    assert call(ok, ctypes.byref(bad), *([p] * 10), None) == 1
    bad = k._terms_struct()
    bad.offset[1] = 1
    assert call(ok, ctypes.byref(bad), *([p] * 10), None) == 1
    assert lib.mfgm_sparse_cond_score_workspace_doubles(1) == 48
    assert lib.mfgm_sparse_cond_score_workspace_doubles(65) == 96


def test_trainer_needs_input_data_and_models_refuse():
    """KernelHyperTrainer asks for input_data with a model trained on its ELBO; a PiecewiseKernel is refused."""
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Gaussian
    from vidp_amd.sparse_variational_cvi import SparseCVIGaussianProcess
    from vidp_amd.trainers import KernelHyperTrainer
    z = torch.linspace(0.0, 5.0, 6, dtype=torch.float64)
    model = SparseCVIGaussianProcess(K.Matern32(1.0, 1.0), z, Gaussian(0.1))
    with pytest.raises(ValueError, match="input_data"):
        KernelHyperTrainer(model)
    tr = KernelHyperTrainer(model, input_data=(z, z[:, None]))
    assert tr.input_data is not None
    pw = K.PiecewiseKernel([K.Matern32(1.0, 1.0), K.Matern32(2.0, 1.0)], torch.tensor([0.5], dtype=torch.float64))
    with pytest.raises(NotImplementedError):
        SparseCVIGaussianProcess(pw, z, Gaussian(0.1)).elbo_and_grad((z, z[:, None]))
