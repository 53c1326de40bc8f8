"""Host tests of the posterior-sampling contract (include/mfgm.h, mfgm_packed_sample) on its NumPy restatement, and the argument
handling that needs no device."""
import numpy as np
import pytest

from oracle import np_btd
from tests import np_sample
from tests.helpers import random_dominant_btd


def test_restatement_whitens_the_draw():
    """(x - mu)^T Lambda (x - mu) = |eps|^2 for every sample and chain, and mu = Lambda^{-1} r."""
    rng = np.random.default_rng(3)
    B, T, d, S = 2, 9, 3, 4
    diag, sub = random_dominant_btd(rng, (B,), T, d)
    r = rng.normal(size=(B, T, d))
    x, e, _, _ = np_sample.sample(diag, sub, r, seed=11, s=1, S=S)
    for b in range(B):
        lam = np_btd.to_dense(diag[b], sub[b])
        mu = np.linalg.solve(lam, r[b].reshape(-1))
        for n in range(S):
            dx = x[n, b].reshape(-1) - mu
            np.testing.assert_allclose(dx @ lam @ dx, np.sum(e[n, b] ** 2), rtol=1e-10)


def test_noise_index_rule():
    """eps[n, b, t] is path n, step b T + t of the stream: a prefix of the samples and independent of B."""
    S, B, T, d = 5, 3, 7, 5
    e = np_sample.eps(42, 1, S, B, T, d)
    np.testing.assert_array_equal(np_sample.eps(42, 1, 2, B, T, d), e[:2])
    np.testing.assert_array_equal(np_sample.eps(42, 1, S, 1, T, d)[:, 0], e[:, 0])
    np.testing.assert_array_equal(np_sample.eps(42, 1, S, 2, T, d), e[:, :2])
    assert np.abs(np_sample.eps(42, 2, S, B, T, d) - e).max() > 0.1
    assert np.abs(np_sample.eps(43, 1, S, B, T, d) - e).max() > 0.1


@pytest.mark.parametrize("shape, expected", [(0, ((0,), 0)), (6, ((6,), 6)), ((10, 10), ((10, 10), 100)), ((3, 1), ((3, 1), 3)),
                                             ((0, 1), ((0, 1), 0)), ((1, 1, 1), ((1, 1, 1), 1)), ([2, 1, 3], ((2, 1, 3), 6))])
def test_sample_shape_normalisation(shape, expected):
    import vidp_amd.sampling as smp
    assert smp.sample_shape_tuple(shape) == expected


def test_argument_errors_without_a_device():
    import vidp_amd.sampling as smp
    with pytest.raises(ValueError):
        smp.sample_shape_tuple((2, -1))
    with pytest.raises(ValueError):
        smp.check_seed(-1, 1)
    with pytest.raises(ValueError):
        smp.check_seed(2 ** 64, 1)
    with pytest.raises(ValueError):
        smp.check_seed(0, 2 ** 32)
    assert smp.check_seed(2 ** 64 - 1, 2) == (2 ** 64 - 1, 2)
