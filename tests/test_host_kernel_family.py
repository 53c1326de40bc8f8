"""
CPU tests of HarmonicOscillator, Constant and Product (vidp_amd.kernels), of Sums holding them and of Matern-only trees: constructor
checks, the torch closed forms against the NumPy restatement tests/np_kernels_ext.py, A against the matrix exponential of the
Kronecker-sum generator, the exact-zero Q of the noise-free kernels, and the f-covariance of the state-space prior against the dense
covariance function.
"""
import numpy as np
import pytest
import torch

from oracle import np_kernels
from tests import np_kernels_ext as E


def kernels_pair(name):
    """(vidp_amd tree, NumPy tree) of the named test kernel."""
    from vidp_amd import kernels as K

    def mk(m, x):
        P, S, HO, C = x.Product, m.Sum, x.HarmonicOscillator, x.Constant
        return {
            "c": lambda: C(1.7),
            "ho": lambda: HO(1.3, 0.8),
            "m52c": lambda: P([m.Matern52(0.9, 1.1), C(0.6)]),
            "m32ho": lambda: P([m.Matern32(0.7, 1.3), HO(1.0, 1.5)]),
            "m52_m12ho": lambda: S([m.Matern52(0.5, 1.0), P([m.Matern12(0.8, 2.0), HO(0.7, 0.6)])]),
            "m52ho": lambda: P([m.Matern52(1.2, 0.9), HO(1.0, 2.5)]),
            "m32ho_m52": lambda: S([P([m.Matern32(0.4, 0.5), HO(1.0, 1.1)]), m.Matern52(2.0, 1.5)]),
            "hom32ho": lambda: P([HO(1.0, 3.0), m.Matern32(1.5, 0.8), HO(0.5, 0.7)]),
            "m52ho_m52": lambda: S([P([m.Matern52(1.2, 0.9), HO(1.0, 2.5)]), m.Matern52(0.3, 0.4)]),
            "m52ho_m32ho": lambda: S([P([m.Matern52(1.2, 0.9), HO(1.0, 2.5)]), P([m.Matern32(0.6, 1.4), HO(2.0, 0.4)])]),
            "d11": lambda: S([P([m.Matern52(1.2, 0.9), HO(1.0, 2.5)]), P([m.Matern32(0.6, 1.4), HO(2.0, 0.4)]), C(0.3)]),
            "d12": lambda: S([P([m.Matern52(1.2, 0.9), HO(1.0, 2.5)]), P([m.Matern52(0.4, 0.3), HO(0.5, 0.9)])]),
            "sum_x_ho": lambda: P([S([m.Matern12(0.5, 1.0), m.Matern32(1.0, 0.5)]), HO(1.0, 1.7)]),
            "m32m52": lambda: P([m.Matern32(0.9, 1.2), m.Matern52(1.4, 0.7)]),
            "m32cho": lambda: P([m.Matern32(0.9, 1.2), C(2.0), HO(0.8, 1.3)]),
            "ou_c_ho": lambda: S([m.OrnsteinUhlenbeck(1.3, 0.6), C(0.5), HO(1.0, 4.0)]),
            # Matern-only trees: the same closed forms, device-built by k_stationary_ssm up to d = 8
            "m12": lambda: m.Matern12(0.8, 2.0),
            "m32": lambda: m.Matern32(0.7, 1.3),
            "m52": lambda: m.Matern52(1.4, 0.7),
            "m12_m32_m52": lambda: S([m.Matern12(0.8, 2.0), m.Matern32(0.7, 1.3), m.Matern52(1.4, 0.7)]),
            # (variances that sum to 9: each of the 39 transitions of the f-covariance test adds up to 3 jitters to var f, 1.2e-4 in all,
            #  and that test allows 1e-5 (max |k| + |k|) = 1.8e-4 on the diagonal)
            "m52x3": lambda: S([m.Matern52(1.4, 2.0), m.Matern52(0.3, 4.0), m.Matern52(2.5, 3.0)]),
        }[name]()
    return mk(K, K), mk(np_kernels, E)


DIMS = {"c": 1, "ho": 2, "m52c": 3, "m32ho": 4, "m52_m12ho": 5, "m52ho": 6, "m32ho_m52": 7, "hom32ho": 8, "m52ho_m52": 9,
        "m52ho_m32ho": 10, "d11": 11, "d12": 12, "sum_x_ho": 6, "m32m52": 6, "m32cho": 4, "ou_c_ho": 4,
        "m12": 1, "m32": 2, "m52": 3, "m12_m32_m52": 6, "m52x3": 9}


def test_constructor_checks_match_the_reference():
    from vidp_amd import kernels as K
    with pytest.raises(ValueError, match="variance must be positive."):
        K.HarmonicOscillator(0.0, 1.0)
    with pytest.raises(ValueError, match="period must be positive."):
        K.HarmonicOscillator(1.0, -2.0)
    with pytest.raises(ValueError, match="variance must be positive."):
        K.Constant(-1.0)
    with pytest.raises(AssertionError, match="There must be at least one child kernel."):
        K.Product([])
    with pytest.raises(TypeError, match="can only combine Kernel instances"):
        K.Product([K.Matern12(1.0, 1.0), 3.0])
    k = K.Product([K.Matern52(1.0, 1.0), K.HarmonicOscillator(1.0, 1.0), K.Constant(2.0)], jitter=1e-6)
    assert k.state_dim == 6 and k.jitter == 1e-6 and k.output_dim == 1


@pytest.mark.parametrize("name", sorted(DIMS))
@pytest.mark.parametrize("jitter", [0.0, 1e-6])
def test_closed_forms_match_numpy(rng, name, jitter):
    """transition_statistics_local, Pinf, H, the feedback matrix and the initial moments against np_kernels_ext within 1e-13 of max |Pinf|,
    on gaps 0, 1e-9, O(1) and many periods."""
    gk, ok = kernels_pair(name)
    gk.jitter = ok.jitter = jitter
    assert gk.state_dim == ok.state_dim == DIMS[name]
    dt = np.concatenate([[0.0, 1e-9, 1e-4], rng.uniform(0.0, 2.0, size=20), [37.3, 123.456]])
    A, Q = gk.transition_statistics_local(torch.from_numpy(dt))
    oA, oQ = ok.transition_statistics(dt)
    Pinf = ok.steady_state_covariance()
    scale = np.abs(Pinf).max()
    np.testing.assert_allclose(gk.steady_state_covariance.numpy(), Pinf, rtol=0, atol=1e-13 * scale)
    np.testing.assert_allclose(A.numpy(), oA, rtol=0, atol=1e-13 * max(1.0, np.abs(oA).max()))
    np.testing.assert_allclose(Q.numpy(), oQ, rtol=0, atol=1e-13 * scale)
    np.testing.assert_allclose(gk.feedback_matrix.numpy(), ok.feedback_matrix(), rtol=1e-14, atol=0)
    np.testing.assert_allclose(gk.initial_covariance_matrix().numpy(), ok.initial_covariance(), rtol=0, atol=1e-13 * scale)
    np.testing.assert_array_equal(gk.initial_mean(()).numpy(), np.zeros(gk.state_dim))
    np.testing.assert_array_equal(gk._emission_row().numpy()[None], ok.emission_vector())


def test_transition_is_the_exponential_of_the_kronecker_sum():
    """A = expm((F1 (+) F2) dt) for Product(Matern32, HarmonicOscillator), with F1 (+) F2 = F1 (x) I + I (x) F2; feedback_matrix itself
    is F1 (x) F2, as in the reference."""
    from vidp_amd import kernels as K
    m, h = K.Matern32(0.7, 1.3), K.HarmonicOscillator(1.0, 1.5)
    k = K.Product([m, h])
    F1, F2 = m.feedback_matrix, h.feedback_matrix
    G = torch.kron(F1, torch.eye(2, dtype=torch.float64)) + torch.kron(torch.eye(2, dtype=torch.float64), F2)
    dt = torch.tensor([0.0, 0.01, 0.3, 1.0, 4.2], dtype=torch.float64)
    A, _ = k.transition_statistics_local(dt)
    np.testing.assert_allclose(A.numpy(), torch.linalg.matrix_exp(G * dt[:, None, None]).numpy(), rtol=0, atol=1e-13)
    np.testing.assert_array_equal(k.feedback_matrix.numpy(), torch.kron(F1, F2).numpy())


@pytest.mark.parametrize("name", ["ho", "c", "hoxc", "hoxho"])
def test_noise_free_kernels_have_exactly_zero_q(name):
    from vidp_amd import kernels as K
    k = {"ho": lambda: K.HarmonicOscillator(1.3, 0.8), "c": lambda: K.Constant(2.5),
         "hoxc": lambda: K.Product([K.HarmonicOscillator(1.3, 0.8), K.Constant(2.5)]),
         "hoxho": lambda: K.Product([K.HarmonicOscillator(1.3, 0.8), K.HarmonicOscillator(0.5, 2.1)])}[name]()
    dt = torch.tensor([0.0, 1e-7, 0.123, 1.7, 55.5], dtype=torch.float64)
    A, Q = k.transition_statistics_local(dt)
    assert bool((Q == 0).all())
    assert k._parts(dt)[3]
    # with a jitter, Q is exactly the jitter
    k.jitter = 1e-6
    np.testing.assert_array_equal(k.transition_statistics_local(dt)[1].numpy(), np.broadcast_to(1e-6 * np.eye(k.state_dim), Q.shape))


def test_quasi_periodic_q_is_the_matern_q_times_the_oscillator_variance():
    """Exactly one factor with M != P: Q = Q_Matern (x) sigma^2 I, no more cancellation than the Matern alone."""
    from vidp_amd import kernels as K
    m = K.Matern52(0.8, 1.4)
    k = K.Product([m, K.HarmonicOscillator(0.7, 1.9)])
    dt = torch.tensor([1e-6, 0.01, 0.5, 3.0], dtype=torch.float64)
    _, Qm = m.transition_statistics_local(dt)
    _, Q = k.transition_statistics_local(dt)
    np.testing.assert_allclose(Q.numpy(), E.kron(Qm.numpy(), 0.7 * np.eye(2)), rtol=1e-14, atol=0)
    assert bool((Q[:, 0:3:2, 1:4:2] == 0).all())   # the oscillator's off-diagonal stays exactly zero


F_COV_CASES = ([(n, 0.0) for n in ["c", "ho", "m32ho", "m52_m12ho", "m52ho", "hom32ho", "d12", "sum_x_ho", "m32m52", "m32cho", "ou_c_ho",
                                          "m12_m32_m52", "m52x3"]]
               # with a jitter only trees whose every term has a Matern factor: a noise-free term integrates the jitter as a random walk
               # (checked on its own below)
               + [(n, 1e-6) for n in ["m32ho", "m52_m12ho", "m52ho", "d12", "sum_x_ho", "m32m52", "m32cho", "m12_m32_m52", "m52x3"]])


@pytest.mark.parametrize("name,jitter", F_COV_CASES)
def test_f_covariance_equals_the_dense_kernel(rng, name, jitter):
    """H Sigma(t_i, t_j) H^T of the torch closed forms equals k(t_i - t_j) (rtol 1e-10 without jitter; 1e-5 with jitter 1e-6, as the
    reference's tests/integration/test_f_covariance.py)."""
    gk, ok = kernels_pair(name)
    gk.jitter = jitter
    t = np.sort(rng.uniform(0.0, 6.0, size=40))
    A, Q = gk.transition_statistics_local(torch.from_numpy(np.diff(t)))
    K = E.f_covariance(A.numpy(), Q.numpy(), gk.initial_covariance_matrix().numpy(), gk._emission_row().numpy()[None])
    dense = E.dense_k(ok, t[:, None] - t[None, :])
    scale = np.abs(dense).max()
    if jitter == 0.0:
        np.testing.assert_allclose(K, dense, rtol=1e-10, atol=1e-10 * scale)
    else:
        np.testing.assert_allclose(K, dense, rtol=1e-5, atol=1e-5 * scale)


def test_jitter_on_a_noise_free_kernel_is_a_random_walk(rng):
    """HarmonicOscillator with jitter j: Q = j I and A orthogonal, so Sigma(t_i, t_i) = (variance + (i + 1) j) I exactly in exact arithmetic."""
    from vidp_amd import kernels as K
    k = K.HarmonicOscillator(1.3, 0.8, jitter=1e-6)
    t = np.sort(rng.uniform(0.0, 6.0, size=40))
    A, Q = k.transition_statistics_local(torch.from_numpy(np.diff(t)))
    Kf = E.f_covariance(A.numpy(), Q.numpy(), k.initial_covariance_matrix().numpy(), k._emission_row().numpy()[None])
    np.testing.assert_allclose(np.diag(Kf), 1.3 + 1e-6 * np.arange(1, 41), rtol=1e-13)


def test_oracle_restatement_f_covariance_equals_the_dense_kernel(rng):
    """The NumPy restatement is itself pinned to the dense known answer (the literal Q carries O(eps) residue for the oscillator)."""
    for name in ("m32ho", "m52_m12ho", "sum_x_ho", "m32cho"):
        _, ok = kernels_pair(name)
        t = np.sort(rng.uniform(0.0, 6.0, size=30))
        dense = E.dense_k(ok, t[:, None] - t[None, :])
        np.testing.assert_allclose(E.ssm_f_covariance(ok, t), dense, rtol=1e-9, atol=1e-9 * np.abs(dense).max())


def test_terms_and_routes():
    """Which trees the term struct expresses: Sums of up to 8 products of up to 3 primitive factors; a Product with a Sum child or more
    than 3 factors takes the torch route."""
    from vidp_amd import _lib, kernels as K
    qp = K.Product([K.Matern32(1.0, 1.0), K.HarmonicOscillator(2.0, 3.0)])
    assert qp._terms() == [[(_lib.FACTOR_MATERN32, np.sqrt(3.0), 1.0), (_lib.FACTOR_HARMONIC, 2 * np.pi / 3.0, 2.0)]]
    assert K.Sum([K.Matern12(1.0, 1.0), qp])._terms()[0] == [(_lib.FACTOR_MATERN12, 1.0, 1.0)]
    assert not K.Sum([K.Matern12(1.0, 1.0), qp])._matern_tree and K.Sum([K.Matern12(1.0, 1.0)])._matern_tree
    assert K.Product([K.Sum([K.Matern12(1.0, 1.0), K.Matern12(2.0, 1.0)]), K.HarmonicOscillator(1.0, 1.0)])._terms() is None
    assert K.Product([K.Constant(1.0)] * 4)._terms() is None
    assert K.Product([K.Product([K.Constant(1.0), K.Matern12(1.0, 1.0)]), K.HarmonicOscillator(1.0, 1.0)])._terms() is not None
