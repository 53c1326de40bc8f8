"""
Host tests of the latent exponentially generated kernel (vidp_amd.kernels.LatentExponentiallyGenerated): the NumPy restatement
tests/np_leg.py against an eigendecomposition route and against a closed-form covariance, the fp64 restatement of the device
exponential against the long-double one, the class on CPU tensors (matrices, _parts, validation, leaves, Sum / Product), and the
argument checks of the two entry points.  No GPU.
"""
import ctypes

import numpy as np
import pytest

from oracle import np_kernels
from tests import np_kernels_ext as E
from tests import np_leg as L


def _random_leg(rng, d, shift=True):
    return rng.random((d, d)) + (np.eye(d) if shift else 0.0), rng.random((d, d))


@pytest.mark.parametrize("d", range(1, 9))
def test_longdouble_expm_against_eigendecomposition(rng, d):
    """The oracle's exponential against V exp(Lambda) V^-1, to 1e-13 (measured 1.8e-15)."""
    N, R = _random_leg(rng, d)
    F = L.LatentExponentiallyGenerated(N, R).feedback_matrix()
    for dt in (0.0, 1e-3, 0.3, 2.0):
        got, want = L.expm(F * dt), L.expm_eig(F * dt)
        print(f"d={d} dt={dt} max|diff|={np.abs(got - want).max():.3e}")
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-13)


def test_device_algorithm_in_fp64_against_longdouble(rng):
    """The arithmetic of leg_expm restated in fp64 (adaptive degree <= 18, scaling to |X|_1 <= 1/2) against the degree-30 long-double
    series on d <= 8, N, R ~ U[0, 1) and gaps in [1e-6, 41] and 0: A and I - A A^T within 1e-13 (measured 4.1e-15 and 5.8e-15), so the
    GPU tests' 1e-12 leaves two orders for the order of the fused multiply-adds; the degree never reaches the cap; dt = 0 is exact."""
    worst_a = worst_q = 0.0
    for d in range(1, 9):
        for rep in range(4):
            N, R = _random_leg(rng, d, shift=bool(rep % 2))
            F = L.LatentExponentiallyGenerated(N, R).feedback_matrix()
            for dt in np.concatenate([[0.0], 10.0 ** rng.uniform(-6.0, np.log10(41.0), size=12)]):
                A, m, s = L.device_expm(F, dt)
                Al = L.expm_ld(F * dt)
                Ql = (np.eye(d, dtype=np.longdouble) - Al @ Al.T).astype(np.float64)
                worst_a = max(worst_a, np.abs(A - Al.astype(np.float64)).max())
                worst_q = max(worst_q, np.abs(np.eye(d) - A @ A.T - Ql).max())
                assert 1 <= m <= 16 and 0 <= s <= 13
                if dt == 0.0:
                    np.testing.assert_array_equal(A, np.eye(d))
    print(f"max|A - A_ld|={worst_a:.3e} max|Q - Q_ld|={worst_q:.3e}")
    assert worst_a <= 1e-13 and worst_q <= 1e-13


def _damped_cosine(lam, omega):
    return np.sqrt(2.0 * lam) * np.eye(2), np.array([[0.0, omega], [0.0, 0.0]])


def test_known_answer_damped_cosine():
    """N = sqrt(2 lam) I, R = [[0, omega], [0, 0]]: F = -lam I - (omega / 2) J, k(tau) = exp(-lam |tau|) cos(omega tau / 2)."""
    lam, omega = 0.7, 2.6
    k = L.LatentExponentiallyGenerated(*_damped_cosine(lam, omega))
    np.testing.assert_allclose(L.dense_k(k, 0.37), 0.68424634868256, rtol=0, atol=1e-14)
    tau = np.array([-3.0, -0.37, 0.0, 1e-4, 0.37, 2.0, 11.0])
    np.testing.assert_allclose(L.dense_k(k, tau), np.exp(-lam * np.abs(tau)) * np.cos(0.5 * omega * tau), rtol=0, atol=1e-14)
    # the SSM of the restatement reproduces the dense covariance
    t = np.array([0.0, 0.2, 0.9, 1.0, 2.7])
    np.testing.assert_allclose(E.ssm_f_covariance(k, t), L.dense_k(k, t[:, None] - t[None, :]), rtol=0, atol=1e-13)


@pytest.mark.parametrize("d", [1, 3, 8, 10])
def test_class_on_cpu_tensors(rng, d):
    """feedback_matrix, steady_state_covariance, _parts, the emission row and transition_statistics_local (CPU tensors: the torch
    route) against np_leg to 1e-12."""
    import torch
    from vidp_amd import kernels as K
    N, R = _random_leg(rng, d)
    gk, ok = K.LatentExponentiallyGenerated(N, R, jitter=1e-6), L.LatentExponentiallyGenerated(N, R, jitter=1e-6)
    assert gk.state_dim == d and gk.output_dim == 1 and gk._terms() is None
    np.testing.assert_allclose(gk.feedback_matrix.numpy(), ok.feedback_matrix(), rtol=0, atol=1e-14)
    np.testing.assert_array_equal(gk.steady_state_covariance.numpy(), np.eye(d))
    dt = np.array([[0.0, 1e-3, 0.3], [2.0, 17.3, 0.05]])
    A, P, Qt, exact = gk._parts(torch.from_numpy(dt))
    oA, oQ = ok.transition_statistics(dt)
    assert not exact
    np.testing.assert_allclose(A.numpy(), oA, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(P.numpy(), np.eye(d))
    np.testing.assert_allclose(Qt.numpy() + 1e-6 * np.eye(d), oQ, rtol=0, atol=1e-12)
    lA, lQ = gk.transition_statistics_local(torch.from_numpy(dt))
    np.testing.assert_allclose(lA.numpy(), oA, rtol=0, atol=1e-12)
    np.testing.assert_allclose(lQ.numpy(), oQ, rtol=0, atol=1e-12)
    h = np.zeros(d)
    h[0] = 1.0
    np.testing.assert_array_equal(gk._emission_row().numpy(), h)
    np.testing.assert_array_equal(gk.initial_covariance_matrix().numpy(), (1.0 + 1e-6) * np.eye(d))
    m = rng.normal(size=d)
    gk.set_state_mean(m)
    np.testing.assert_array_equal(gk.state_mean.numpy(), m)
    B = rng.normal(size=d)
    gb = K.LatentExponentiallyGenerated(N, R, emission=B)
    np.testing.assert_array_equal(gb._emission_row().numpy(), B)
    np.testing.assert_array_equal(gb.generate_emission_model(torch.zeros(4, dtype=torch.float64)).emission_matrix.numpy(),
                                  np.broadcast_to(B, (4, 1, d)))


def test_argument_validation():
    from vidp_amd import kernels as K
    for N, R in [(np.ones((2, 3)), np.ones((2, 3))), (np.ones((2, 2)), np.ones((3, 3))), (np.ones(3), np.ones(3)),
                 (np.ones((0, 0)), np.ones((0, 0)))]:
        with pytest.raises(ValueError, match="square"):
            K.LatentExponentiallyGenerated(N, R)
    with pytest.raises(ValueError, match="emission"):
        K.LatentExponentiallyGenerated(np.eye(2), np.eye(2), emission=[1.0, 0.0, 0.0])
    with pytest.raises(ValueError, match="state_dim <= 8"):
        K.LatentExponentiallyGenerated(np.eye(9), np.eye(9))._spec()


def test_leaves_are_differentiable(rng):
    """hyperparameter_leaves: N and R [d, d] with requires_grad (the emission is not a leaf); _parts on them is differentiable and
    d A / d N agrees with a central difference."""
    import torch
    from vidp_amd import kernels as K
    N, R = _random_leg(rng, 3)
    gk = K.LatentExponentiallyGenerated(N, R, emission=[1.0, 0.5, 0.0])
    lv = gk.hyperparameter_leaves()
    assert sorted(lv) == ["N", "R"] and all(v.requires_grad and tuple(v.shape) == (3, 3) for v in lv.values())
    np.testing.assert_array_equal(lv["N"].detach().numpy(), N)
    dt = torch.tensor([0.3, 1.1], dtype=torch.float64)
    w = torch.from_numpy(rng.normal(size=(2, 3, 3)))
    f = lambda l: (gk._parts(dt, l)[0] * w).sum() + (gk._parts(dt, l)[2] * w).sum()
    gN, gR = torch.autograd.grad(f(lv), [lv["N"], lv["R"]])
    for name, g in (("N", gN), ("R", gR)):
        for i, j in [(0, 0), (1, 2), (2, 1)]:
            def at(e):
                l = {k: v.detach().clone() for k, v in lv.items()}
                l[name][i, j] += e
                return float(f(l))
            np.testing.assert_allclose(float(g[i, j]), (at(1e-6) - at(-1e-6)) / 2e-6, rtol=1e-6, atol=1e-9)


def test_sum_and_product_take_a_leg_child(rng):
    """Sum([LEG, Matern32]) and Product([LEG, HarmonicOscillator]) _parts against the NumPy block-diagonal / Kronecker forms."""
    import torch
    from vidp_amd import kernels as K
    N, R = _random_leg(rng, 2)
    dt = np.array([0.0, 0.01, 0.4, 3.0])
    gs = K.Sum([K.LatentExponentiallyGenerated(N, R), K.Matern32(0.8, 1.3)])
    os_ = np_kernels.Sum([L.LatentExponentiallyGenerated(N, R), np_kernels.Matern32(0.8, 1.3)])
    gp = K.Product([K.LatentExponentiallyGenerated(N, R), K.HarmonicOscillator(1.2, 0.9)])
    op = E.Product([L.LatentExponentiallyGenerated(N, R), E.HarmonicOscillator(1.2, 0.9)])
    for gk, ok in ((gs, os_), (gp, op)):
        assert gk.state_dim == 4 and gk._terms() is None
        A, P, Qt, exact = gk._parts(torch.from_numpy(dt))
        oA, oQ = ok.transition_statistics(dt)
        assert not exact
        np.testing.assert_allclose(A.numpy(), oA, rtol=0, atol=1e-12)
        np.testing.assert_allclose(np.broadcast_to(P.numpy(), (4, 4)), ok.steady_state_covariance(), rtol=0, atol=1e-12)
        np.testing.assert_allclose(Qt.numpy(), oQ, rtol=0, atol=1e-12)
        np.testing.assert_array_equal(gk._emission_row().numpy(), ok.emission_vector()[0])


def test_entry_points_check_their_arguments_without_a_gpu():
    """mfgm_packed_leg_ssm and mfgm_leg_transitions return 1, before any HIP call, for d in {0, 9}, null pointers and a plan of
    another state dimension; mfgm_leg_transitions with n = 0 returns 0."""
    import vidp_amd
    lib = vidp_amd._lib.load()
    plan3, plan16 = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.mfgm_plan_create(2, 10, 3, 0, 0, ctypes.byref(plan3)) == 0
    assert lib.mfgm_plan_create(2, 10, 16, 0, 0, ctypes.byref(plan16)) == 0
    p = ctypes.c_void_p(64)        # non-null, never dereferenced by a rejected call
    null = ctypes.c_void_p(0)

    def spec(d):
        s = vidp_amd._lib.LegSpec()
        s.d = d
        return s
    ok = spec(3)
    for d in (0, 9, -1):
        assert lib.mfgm_packed_leg_ssm(plan3, ctypes.byref(spec(d)), p, p, p, p, p, null) == 1
        assert lib.mfgm_leg_transitions(ctypes.byref(spec(d)), 5, p, p, p, null) == 1
        assert lib.mfgm_leg_transitions(ctypes.byref(spec(d)), 0, p, p, p, null) == 1
    assert lib.mfgm_packed_leg_ssm(plan3, ctypes.byref(spec(2)), p, p, p, p, p, null) == 1      # the plan has d = 3
    assert lib.mfgm_packed_leg_ssm(plan16, ctypes.byref(spec(8)), p, p, p, p, p, null) == 1
    assert lib.mfgm_packed_leg_ssm(null, ctypes.byref(ok), p, p, p, p, p, null) == 1
    assert lib.mfgm_packed_leg_ssm(plan3, null, p, p, p, p, p, null) == 1
    for k in range(5):
        args = [p] * 5
        args[k] = null
        assert lib.mfgm_packed_leg_ssm(plan3, ctypes.byref(ok), *args, null) == 1
    assert lib.mfgm_leg_transitions(null, 5, p, p, p, null) == 1
    for k in range(3):
        args = [p] * 3
        args[k] = null
        assert lib.mfgm_leg_transitions(ctypes.byref(ok), 5, *args, null) == 1
    assert lib.mfgm_leg_transitions(ctypes.byref(ok), -1, p, p, p, null) == 1
    assert lib.mfgm_leg_transitions(ctypes.byref(ok), 0, p, p, p, null) == 0
    assert lib.mfgm_leg_transitions(ctypes.byref(ok), 0, null, null, null, null) == 0
    lib.mfgm_plan_destroy(plan3)
    lib.mfgm_plan_destroy(plan16)
