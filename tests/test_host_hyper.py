"""
CPU tests of the hyper-parameter score: the NumPy restatement of csrc/mfgm_score.h (tests/np_hyper.py) against the
dense-covariance gradient, its fp64 rounding against np.longdouble, the conditioning table, the chain rule from the device's
(rate, var) to the kernels' leaves, assign_hyperparameters / hyperparameter_values, the trainer's transforms, the argument checks of
mfgm_packed_kernel_score and the rejection of a noise-free HarmonicOscillator.  No GPU.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import np_hyper as H

T = 40
NOISE = 0.3
BOUND = 1.01e-10      # 10 x the worst restatement-against-dense error measured (test_restatement_against_dense)


def _case(rng, spec, jitter, min_gap=0.5):
    t = H.make_grid(rng, spec, T, min_gap)
    y = rng.normal(size=T)
    return t, y, H.oracle_moments(spec, jitter, t, y, NOISE)


@pytest.mark.parametrize("name,spec,jitter", H.TREES, ids=[n for n, _, _ in H.TREES])
def test_restatement_against_dense(rng, name, spec, jitter):
    """The fp64 restatement on the oracle's pairwise posterior (oracle.np_kalman) against 1/2 tr((alpha alpha^T - K_y^-1) dK) with dK
    by the complex step, T = 40, gaps max(Exp(0.5 l), 0.5 l) with l the tree's shortest time scale.  Worst value measured over the
    thirteen trees, relative to max(1, |g|): 1.01e-11 (sum_m52_m52_m32, whose longest lengthscale makes the gaps 0.19 l there:
    cond Q ~ 5e4); 7.2e-12 for sum_prod_m12_h_const, whose dense K comes from the state-space recursion because of the jitter;
    <= 7e-13 for every tree of state dimension <= 6 without jitter.  Asserted at 10 x the worst value.  The noise gradient
    1/2 tr(alpha alpha^T - K_y^-1) against the f-marginal formula of GaussianProcessRegression.log_likelihood_and_grad is the same
    comparison and takes the same bound (measured <= 1.4e-14, 9.3e-12 for the jitter tree)."""
    t, y, (x, Sig, Sub) = _case(rng, spec, jitter)
    ll, g, gn = H.dense_ll_and_grad(spec, jitter, t, y, NOISE)
    got = H.leaves_from_score(spec, H.score_restatement(spec, jitter, np.diff(t), x, Sig, Sub))
    err = np.max(np.abs(got - g) / np.maximum(1.0, np.abs(g)))
    print(f"{name}: restatement against dense {err:.2e}")
    assert err <= BOUND
    k = H.build_np(spec, jitter)
    h = k.emission_vector().reshape(-1)
    mf = (x + k.state_space_model(t).marginal_means) @ h
    vf = np.einsum("i,tij,j->t", h, Sig, h)
    noise = 0.5 * (((y - mf) ** 2 + vf) / NOISE ** 2 - 1.0 / NOISE).sum()
    print(f"{name}: noise gradient against dense {abs(noise - gn) / max(1.0, abs(gn)):.2e}")
    assert abs(noise - gn) <= BOUND * max(1.0, abs(gn))


def test_closed_form_k_is_the_oracles(rng):
    """np_hyper.k_closed (complex-capable) against tests.np_kernels_ext.dense_k on every jitter-free tree, and the state-space
    k_ssm against it."""
    from tests import np_kernels_ext as E
    for name, spec, jitter in H.TREES:
        if jitter != 0.0:
            continue
        t = H.make_grid(rng, spec, 12)
        r = np.abs(t[:, None] - t[None, :])
        ref = E.dense_k(H.build_np(spec), r)
        np.testing.assert_allclose(H.k_closed(spec, r), ref, rtol=1e-14, atol=1e-15)
        np.testing.assert_allclose(H.k_ssm(spec, 0.0, t, np.float64), ref, rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("name,spec,jitter", H.TREES, ids=[n for n, _, _ in H.TREES])
def test_fp64_against_long_double(rng, name, spec, jitter):
    """The fp64 restatement against the same formulas in np.longdouble on identical inputs: the rounding floor of the formulas, and so
    of the GPU kernel that evaluates them.  Worst spread measured over the thirteen trees: np_hyper.FP64_SPREAD, relative to
    max(1, |g|); the GPU tests allow 10 x that constant.  The spread is a rounding-level quantity that moves with the summation order
    of the BLAS behind oracle_moments, so it is bounded here with a factor 2 of headroom."""
    t, y, (x, Sig, Sub) = _case(rng, spec, jitter)
    a = H.score_restatement(spec, jitter, np.diff(t), x, Sig, Sub)
    b = H.score_restatement(spec, jitter, np.diff(t), x, Sig, Sub, dtype=np.longdouble)
    spread = float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))
    print(f"{name}: fp64 against long double {spread:.2e}")
    assert spread <= 2.0 * H.FP64_SPREAD


def test_conditioning_table(rng):
    """The error of the restatement against the dense gradient as the smallest gap shrinks (Matern-3/2 and -5/2, T = 40): Q^-1 (M - Q) Q^-1
    loses about cond(Q) eps.  Printed (DESIGN.md section 18 holds a copy); asserted: monotone in the gap."""
    for name, spec in (("matern32", H.M32), ("matern52", H.M52)):
        errs = []
        for mg in (0.5, 0.2, 0.05, 1e-3):
            r = np.random.default_rng(5)
            t = H.make_grid(r, spec, T, mg)
            y = r.normal(size=T)
            x, Sig, Sub = H.oracle_moments(spec, 0.0, t, y, NOISE)
            _, g, _ = H.dense_ll_and_grad(spec, 0.0, t, y, NOISE)
            got = H.leaves_from_score(spec, H.score_restatement(spec, 0.0, np.diff(t), x, Sig, Sub))
            k = H.build_np(spec)
            cond = max(np.linalg.cond(q) for q in k.transition_statistics(np.diff(t))[1])
            errs.append(float(np.max(np.abs(got - g) / np.maximum(1.0, np.abs(g)))))
            print(f"{name}: minimum gap {mg:g} l  relative error {errs[-1]:.1e}  cond Q {cond:.1e}")
        assert all(a <= b for a, b in zip(errs, errs[1:])), errs


# -- the package's host side ---------------------------------------------------------------------------------------------------------------
def _flat_terms(terms):
    return [(kind, rate, var) for factors in terms for kind, rate, var in factors]


@pytest.mark.parametrize("name,spec,jitter", H.TREES, ids=[n for n, _, _ in H.TREES])
def test_terms_t_chain_rule(name, spec, jitter):
    """_terms_t(leaves): the values of _terms(), and d(rate, var)/d leaf equal to central differences of _terms() (1e-7 relative: the
    quotient's accuracy at h = 1e-6 of the value) and to the closed forms of np_hyper.leaf_grads."""
    from vidp_amd import hyper
    k = H.build_vidp(spec, jitter)
    leaves = k.hyperparameter_leaves()
    tt = _flat_terms(k._terms_t(leaves))
    ref = _flat_terms(k._terms())
    assert [a[0] for a in tt] == [b[0] for b in ref]
    for (_, r, v), (_, r0, v0) in zip(tt, ref):
        # (torch divides through a reciprocal where Python divides: one unit in the last place)
        assert abs(float(r.detach()) - r0) <= 4.5e-16 * abs(r0) and abs(float(v.detach()) - v0) <= 4.5e-16 * abs(v0)
    flat = hyper.flatten(leaves)
    vals = hyper.flatten(k.hyperparameter_values())
    assert [float(l.detach()) for l in flat] == vals == H.flat_params(spec)
    # a random cotangent on (rate, var): the leaf gradients against the differences of the same contraction
    w = np.random.default_rng(3).normal(size=(len(tt), 2))
    obj = sum(r * w[i, 0] + v * w[i, 1] for i, (_, r, v) in enumerate(tt))
    grads = torch.autograd.grad(obj, flat, allow_unused=True)
    grads = [0.0 if g is None else float(g) for g in grads]
    score = np.zeros((8, 3, 2))
    i = 0
    for c, factors in enumerate(k._terms()):
        for f in range(len(factors)):
            score[c, f] = w[i]
            i += 1
    np.testing.assert_allclose(grads, H.leaves_from_score(spec, score), rtol=1e-13, atol=1e-15)

    def contraction(values):
        k.assign_hyperparameters(hyper.unflatten(k.hyperparameter_values(), list(values)))
        return sum(r * w[i, 0] + v * w[i, 1] for i, (_, r, v) in enumerate(_flat_terms(k._terms())))
    for j, v in enumerate(vals):
        h = 1e-6 * v
        up, dn = list(vals), list(vals)
        up[j], dn[j] = v + h, v - h
        fd = (contraction(up) - contraction(dn)) / (2 * h)
        assert abs(fd - grads[j]) <= 1e-7 * max(1.0, abs(grads[j])), (j, fd, grads[j])
    k.assign_hyperparameters(hyper.unflatten(k.hyperparameter_values(), list(vals)))


def test_assign_round_trip_and_validation():
    from vidp_amd import kernels as K
    k = K.Sum([K.Matern32(1.3, 0.8), K.Product([K.Matern12(0.7, 1.2), K.HarmonicOscillator(1.1, 2.5)]), K.Constant(0.6),
               K.OrnsteinUhlenbeck(0.9, 1.1)], jitter=1e-6)
    v = k.hyperparameter_values()
    assert v == [{"lengthscale": 1.3, "variance": 0.8}, [{"lengthscale": 0.7, "variance": 1.2}, {"variance": 1.1, "period": 2.5}],
                 {"variance": 0.6}, {"decay": 0.9, "diffusion": 1.1}]
    new = [{"lengthscale": 2.0, "variance": 0.5}, [{"lengthscale": 0.4, "variance": 1.0}, {"variance": 0.3, "period": 3.0}],
           {"variance": 0.9}, {"decay": 1.5, "diffusion": 0.2}]
    k.assign_hyperparameters(new)
    assert k.hyperparameter_values() == new
    assert k._terms()[0][0][1] == math.sqrt(3.0) / 2.0 and k._terms()[1][1][1] == 2.0 * math.pi / 3.0
    # tensors are accepted; the leaves' structure is the values' structure
    k.assign_hyperparameters([{n: torch.tensor(x, dtype=torch.float64) for n, x in d.items()} if isinstance(d, dict)
                              else [{n: torch.tensor(x, dtype=torch.float64) for n, x in e.items()} for e in d] for d in v])
    assert k.hyperparameter_values() == v
    for bad in (0.0, -1.0, float("nan")):
        for cls, names in ((K.Matern12, ("lengthscale", "variance")), (K.Matern32, ("lengthscale", "variance")),
                           (K.Matern52, ("lengthscale", "variance")), (K.OrnsteinUhlenbeck, ("decay", "diffusion")),
                           (K.HarmonicOscillator, ("variance", "period"))):
            for n in names:
                kk = cls(1.0, 1.0)
                vals = dict(kk.hyperparameter_values())
                vals[n] = bad
                with pytest.raises(ValueError):
                    kk.assign_hyperparameters(vals)
                assert kk.hyperparameter_values() == {m: 1.0 for m in names}
        with pytest.raises(ValueError):
            K.Constant(1.0).assign_hyperparameters({"variance": bad})
    # a failing child leaves the whole tree as it was
    with pytest.raises(ValueError):
        k.assign_hyperparameters([new[0], new[1], {"variance": -1.0}, new[3]])
    assert k.hyperparameter_values() == v
    with pytest.raises(ValueError):
        k.assign_hyperparameters(new[:3])
    with pytest.raises(ValueError):
        K.Matern32(1.0, 1.0).assign_hyperparameters({"lengthscale": 1.0})
    leg = K.LatentExponentiallyGenerated(torch.eye(3), torch.zeros(3, 3))
    N, R = torch.arange(9.0).reshape(3, 3), torch.ones(3, 3)
    leg.assign_hyperparameters({"N": N, "R": R})
    got = leg.hyperparameter_values()
    assert torch.equal(got["N"], N.double()) and torch.equal(got["R"], R.double())
    assert torch.equal(leg.feedback_matrix, K.LatentExponentiallyGenerated._feedback(N.double(), R.double()))
    with pytest.raises(ValueError):
        leg.assign_hyperparameters({"N": torch.eye(2), "R": torch.eye(2)})


def test_transforms_invert():
    from vidp_amd import hyper
    for name, (fwd, inv, jac) in hyper.TRANSFORMS.items():
        for x in (1e-8, 1e-3, 0.3, 1.0, 7.0, 40.0, 800.0):
            u = inv(x)
            assert abs(fwd(u) - x) <= 1e-14 * x, (name, x)
            h = 1e-6 * max(1.0, abs(u))
            fd = (fwd(u + h) - fwd(u - h)) / (2 * h)
            assert abs(fd - jac(u)) <= 1e-8 * max(abs(jac(u)), 1e-300) + 1e-9 * x, (name, x)
        for u in (-30.0, -1.0, 0.0, 2.0, 50.0):
            assert abs(inv(fwd(u)) - u) <= 1e-9 * max(1.0, abs(u)), (name, u)


def test_kernel_score_argument_checks():
    """mfgm_packed_kernel_score returns 1 before any HIP call: null pointers, a d > 8 plan, a tree mfgm_packed_kernel_ssm rejects."""
    from vidp_amd import _lib, kernels as K
    lib = _lib.load()

    def plan(d):
        h = ctypes.c_void_p()
        assert lib.mfgm_plan_create(2, 9, d, 0, 0, ctypes.byref(h)) == 0
        return h
    p = ctypes.c_void_p(8)        # never dereferenced: every call below is refused first
    k = K.Sum([K.Matern32(1.0, 1.0), K.Matern12(1.0, 1.0)])
    kt = k._terms_struct()
    h3 = plan(3)
    call = lambda pl, terms, *a: lib.mfgm_packed_kernel_score(pl, terms, *a)
    assert call(None, ctypes.byref(kt), p, p, p, p, p, p, p, None) == 1
    assert call(h3, None, p, p, p, p, p, p, p, None) == 1
    for hole in range(7):
        args = [p] * 7
        args[hole] = None
        assert call(h3, ctypes.byref(kt), *args, None) == 1, hole
    h9, h2 = plan(9), plan(2)
    assert call(h9, ctypes.byref(kt), p, p, p, p, p, p, p, None) == 1       # wide plan
    assert call(h2, ctypes.byref(kt), p, p, p, p, p, p, p, None) == 1       # the plan's d is not the tree's
    bad = k._terms_struct()
    bad.kind[0][0] = 9
    assert call(h3, ctypes.byref(bad), p, p, p, p, p, p, p, None) == 1
    bad = k._terms_struct()
    bad.offset[1] = 1
    assert call(h3, ctypes.byref(bad), p, p, p, p, p, p, p, None) == 1
    bad = k._terms_struct()
    bad.nfactor[0] = 4
    assert call(h3, ctypes.byref(bad), p, p, p, p, p, p, p, None) == 1
    for h in (h3, h9, h2):
        lib.mfgm_plan_destroy(h)


def test_noise_free_harmonic_is_rejected():
    """A HarmonicOscillator term without jitter has dA != 0 on an exactly-zero Q: rejected by the host check the models run before
    anything is launched; a jitter, or a Matern factor in the same term, makes it admissible."""
    from vidp_amd import hyper, kernels as K
    for k in (K.HarmonicOscillator(1.0, 2.0), K.Product([K.HarmonicOscillator(1.0, 2.0), K.Constant(0.5)]),
              K.Sum([K.Matern32(1.0, 1.0), K.HarmonicOscillator(1.0, 2.0)])):
        with pytest.raises(ValueError, match="jitter"):
            hyper._check_terms(k, k._terms())
    for k in (K.HarmonicOscillator(1.0, 2.0, jitter=1e-6), K.Product([K.Matern32(1.0, 1.0), K.HarmonicOscillator(1.0, 2.0)]),
              K.Constant(0.5)):
        hyper._check_terms(k, k._terms())
    from vidp_amd.kernels import PiecewiseKernel
    pw = PiecewiseKernel([K.Matern32(1.0, 1.0), K.Matern32(2.0, 1.0)], torch.tensor([0.5], dtype=torch.float64))
    with pytest.raises(NotImplementedError):
        hyper.check_supported(pw)
