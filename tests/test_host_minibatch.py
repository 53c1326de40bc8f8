"""
CPU tests of mini-batch sparse CVI: the restatement tests/np_minibatch.py against the DENSE-covariance
conditionals of the stationary process on a tiny case, its rules for absent points, the batch model against the full-data SparseChain,
and the argument checks of mfgm_sparse_batch_predict_lik / mfgm_sparse_batch_seg, which return before any HIP call.  No GPU.
"""
import ctypes

import numpy as np
import pytest

from tests import np_hyper as H
from tests import np_minibatch as MB
from tests import np_sparse_hyper as S

TREES = {name: (spec, jitter) for name, spec, jitter in H.TREES}
ld = np.longdouble


@pytest.mark.parametrize("tree", ["matern32", "matern52", "sum_m52_m32", "prod_m32_h"])
def test_rows_are_the_dense_conditionals(rng, tree):
    """w, c of batch_rows against  f(t) | s(z-), s(z+)  from the stationary covariances Cov(s(a), s(b)) = A(a - b) Pinf (a > b) of the
    same kernel without jitter, both in long double, on unsorted points in the interior and in both end intervals (one conditioning
    state there).  Bound 1e-14 of max(1, |row|): both sides lose eps_ld cond(K_pair) ~ 1e-19 * 1e4 on these gaps; measured 2.0e-18 at worst."""
    spec = TREES[tree][0]
    d = H.state_dim(spec)
    h = S.emission(spec, ld)
    z = np.array([0.0, 1.1, 2.6, 3.4])
    t = np.array([2.9, -0.7, 1.7, 4.2, 0.4, 3.1])
    idx, w, c = MB.batch_rows(spec, 0.0, z, t, ld)
    assert idx.tolist() == [3, 0, 2, 4, 1, 3]
    worst = 0.0
    for i, ti in enumerate(t):
        m = idx[i]
        P = S.transition(spec, 0.0, 0.0, ld)[2]
        blocks, cross = [], []          # the conditioning states present, Cov(s(t), state)
        if m > 0:
            blocks.append("lo")
            cross.append(S.transition(spec, 0.0, ti - z[m - 1], ld)[0] @ P)
        if m < len(z):
            blocks.append("hi")
            cross.append(P @ S.transition(spec, 0.0, z[m] - ti, ld)[0].T)
        if len(blocks) == 2:
            A = S.transition(spec, 0.0, z[m] - z[m - 1], ld)[0]
            Kp = np.block([[P, P @ A.T], [A @ P, P]])
        else:
            Kp = P
        Ks = np.concatenate(cross, axis=1)
        Wf = S.spd_solve(Kp, Ks.T).T
        want_w = np.zeros(2 * d, dtype=ld)
        row = h @ Wf
        if blocks == ["lo", "hi"]:
            want_w[:] = row
        elif blocks == ["lo"]:
            want_w[:d] = row
        else:
            want_w[d:] = row
        want_c = h @ (P - Wf @ Ks.T) @ h
        sc = max(1.0, float(np.abs(want_w).max()), float(abs(want_c)))
        worst = max(worst, float(np.abs(w[i] - want_w).max()) / sc, float(abs(c[i] - want_c)) / sc)
    print(f"{tree}: rows against the dense conditionals {worst:.2e} (bound 1e-14)")
    assert worst <= 1e-14


def test_pass_rules_for_absent_points(rng):
    """A NaN observation: ve = g1 = g2 = 0, fmu / fvar as for any point.  A non-finite time: idx 0, zero row, fmu = shift, fvar = 0,
    zero ve, g1, g2.  kind 0: no likelihood outputs.  ve_sum is the sum of ve."""
    spec, jitter = TREES["sum_m52_m32"]
    d, M = H.state_dim(spec), 4
    z = np.array([0.0, 1.0, 2.2, 3.0])
    t = np.array([1.5, np.nan, -0.3, np.inf, 2.2, 0.6])
    y = np.array([0.3, 0.1, np.nan, 0.2, -0.4, 1.0])
    shift = rng.normal(size=len(t))
    A = rng.normal(size=(M, d, d))
    mu, Sig, Sub = rng.normal(size=(M, d)), A @ A.transpose(0, 2, 1) + np.eye(d), 0.1 * rng.normal(size=(M, d, d))
    P0 = S.transition(spec, jitter, 0.0, np.float64)[2]
    r = MB.batch_pass(spec, jitter, z, t, mu, Sig, Sub, np.zeros(d), P0, ("gaussian", 0.3), y, 2.5, shift, dtype=np.float64)
    assert r["idx"].tolist() == [2, 0, 0, 0, 2, 1]
    for i in (1, 3):
        assert not r["w"][i].any() and r["c"][i] == 0 and r["fmu"][i] == shift[i] and r["fvar"][i] == 0
    for i in (1, 2, 3):
        assert r["ve"][i] == 0 and r["g1"][i] == 0 and r["g2"][i] == 0
    assert r["w"][2].any() and r["fvar"][2] > 0
    # ON an inducing point: the state on the right alone, read through the emission row (one entry per term)
    np.testing.assert_allclose(r["w"][4], np.concatenate([np.zeros(d), S.emission(spec, np.float64)]), atol=1e-12)
    assert abs(r["c"][4]) <= 1e-12
    assert r["ve_sum"] == r["ve"].sum() and r["ve_sum"] != 0
    # the gradients are those of the zero-mean part: g1 = scale (dmu - 2 dv (fmu - shift))
    i, v = 0, 0.3
    assert np.isclose(r["g1"][i], 2.5 * ((y[i] - r["fmu"][i]) / v + (r["fmu"][i] - shift[i]) / v), rtol=1e-13)
    p = MB.batch_pass(spec, jitter, z, t, mu, Sig, Sub, np.zeros(d), P0, dtype=np.float64)
    assert "ve" not in p and np.allclose(p["fmu"], r["fmu"] - shift, rtol=0, atol=1e-14)
    assert MB.batch_seg(z, np.sort(t)).tolist() == [0, 1, 2, 4, 4, 6]       # (np.sort leaves inf, NaN last)


@pytest.mark.parametrize("lik", [("gaussian", 0.3), ("poisson", 0.7), ("bernoulli", 1e-3)])
def test_one_whole_batch_is_the_full_data_model(rng, lik):
    """With the whole data set as one shuffled batch and num_data = N the batch model is SparseChain on the sorted data: the bound and
    one site update agree to 1e-12 (the order of the sums differs); with num_data = 3 N the expectation term and the site target
    are three times as large."""
    spec, jitter = TREES["matern32"]
    z, t, y = S.make_problem(rng, spec, 5, 20, "poisson" if lik[0] == "poisson" else "gaussian")
    if lik[0] == "bernoulli":
        y = (y > 0).astype(np.float64)
    perm = rng.permutation(len(t))
    b1 = MB.BatchChain(spec, jitter, z, t[perm], y[perm], lik, len(t))
    n1, n2 = b1.update_sites(*b1.zero_sites(), 0.5)
    if lik[0] != "bernoulli":
        full = S.SparseChain(spec, jitter, z, t, y, lik)
        f1, f2 = full.update_sites(*full.zero_sites(), 0.5)
        assert np.abs(n1 - f1).max() <= 1e-12 * np.abs(f1).max() and np.abs(n2 - f2).max() <= 1e-12 * np.abs(f2).max()
        assert abs(b1.elbo(n1, n2) - full.elbo(n1, n2)) <= 1e-12 * abs(full.elbo(n1, n2))
    b3 = MB.BatchChain(spec, jitter, z, t[perm], y[perm], lik, 3 * len(t))
    m1, m2 = b3.update_sites(*b3.zero_sites(), 0.5)
    np.testing.assert_allclose(m1, 3.0 * n1, rtol=1e-13, atol=1e-300)
    np.testing.assert_allclose(m2, 3.0 * n2, rtol=1e-13, atol=1e-300)
    zero = b1.zero_sites()
    np.testing.assert_allclose(b3.elbo(*zero), 3.0 * b1.elbo(*zero), rtol=1e-12)       # KL = 0 at zero sites


def test_argument_checks_need_no_gpu():
    """mfgm_sparse_batch_predict_lik returns 1 before any HIP call for a null required argument, M < 1, n < 0, an unknown kind, a
    parameter out of range, a scale that is not finite and positive, likelihood outputs with kind 0, d > 8 and terms
    mfgm_packed_kernel_ssm rejects; n = 0 without ve_sum returns 0 and launches nothing.  mfgm_sparse_batch_seg likewise."""
    import vidp_amd
    from vidp_amd import kernels as K
    lib = vidp_amd._lib.load()
    assert [lib.mfgm_sparse_batch_workspace_doubles(n) for n in (0, 1, 64, 65, 130)] == [1, 1, 1, 2, 3]
    kt = K.Sum([K.Matern52(1.0, 1.0), K.Matern32(0.5, 2.0)])._terms_struct()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # terms, M, z, n, t, shift, kind, param, scale, y, pm, pc, mu, Sig, Sub, idx, w, c, fmu, fvar, ve, g1, g2, ve_sum, ws, info, stream
    good = [ctypes.byref(kt), 3, p, 0, p, None, 0, 0.0, 1.0, None, p, p, p, p, p, None, None, None, p, p, None, None, None, None, None, p, None]
    call = lambda changes={}: lib.mfgm_sparse_batch_predict_lik(*[changes.get(i, a) for i, a in enumerate(good)])
    assert call() == 0                                   # n = 0: nothing to do
    for pos in (0, 2, 10, 11, 12, 13, 14, 25):
        assert call({pos: None}) == 1                    # a null required argument
    assert call({1: 0}) == 1 and call({3: -1}) == 1
    assert call({3: 5, 4: None}) == 1                    # points without times
    assert call({6: 4}) == 1 and call({6: -1}) == 1      # unknown kinds
    for pos in (9, 20, 21, 22, 23):
        assert call({pos: p}) == 1                       # kind 0 takes no observations and no likelihood outputs
    lik = {6: 3, 7: 0.5, 9: p}
    assert call(lik) == 0
    assert call({**lik, 7: 0.0}) == 1 and call({**lik, 7: float("inf")}) == 1 and call({**lik, 7: float("nan")}) == 1
    assert call({**lik, 6: 1, 7: 0.5}) == 1 and call({**lik, 6: 1, 7: -0.1}) == 1 and call({**lik, 6: 1, 7: 0.0}) == 0
    assert call({**lik, 6: 2, 7: 0.0}) == 1
    for s in (0.0, -1.0, float("inf"), float("nan")):
        assert call({**lik, 8: s}) == 1
    assert call({**lik, 3: 5, 9: None}) == 1             # points without observations
    assert call({**lik, 23: p}) == 1                     # ve_sum without a workspace
    bad = K.Sum([K.Matern52(1.0, 1.0), K.Matern32(0.5, 2.0)])._terms_struct()
    bad.offset[1] = 2
    assert call({0: ctypes.byref(bad)}) == 1
    wide = K.Sum([K.Matern52(1.0, 1.0), K.Matern52(0.5, 2.0)])._terms_struct()
    wide.nterm, wide.nfactor[2], wide.offset[2], wide.kind[2][0] = 3, 1, 6, vidp_amd._lib.FACTOR_MATERN52      # d = 9
    assert call({0: ctypes.byref(wide)}) == 1
    seg = lambda M, z, n, t, out: lib.mfgm_sparse_batch_seg(M, z, n, t, out, None)
    assert seg(0, p, 0, p, p) == 1 and seg(3, None, 0, p, p) == 1 and seg(3, p, -1, p, p) == 1 and seg(3, p, 0, p, None) == 1
    assert seg(3, p, 4, None, p) == 1 and seg(3, p, 2 ** 31, p, p) == 1
