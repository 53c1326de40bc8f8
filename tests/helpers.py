"""Random problem generators shared by the oracle and GPU parity tests."""
import numpy as np


def random_spd_btd(rng, batch, T, d, with_sub=True):
    """
    Positive-definite block-tri-diagonal (diag, sub) as in the reference's
    tests/unit/test_block_tri_diag.py:274-296: build a random lower block-bidiagonal L and form L L^T.
    """
    Ld = np.tril(0.5 * rng.normal(size=batch + (T, d, d)))
    idx = np.arange(d)
    Ld[..., idx, idx] = np.abs(Ld[..., idx, idx]) + 1.0
    Ls = 0.5 * rng.normal(size=batch + (T - 1, d, d)) if (with_sub and T > 1) else None
    diag = Ld @ np.swapaxes(Ld, -1, -2)
    sub = None
    if Ls is not None:
        diag[..., 1:, :, :] += Ls @ np.swapaxes(Ls, -1, -2)
        sub = Ls @ np.swapaxes(Ld[..., :-1, :, :], -1, -2)
    return diag, sub, Ld, Ls


def random_dominant_btd(rng, batch, T, d):
    """
    Well-conditioned SPD block-tri-diagonal (cond ~ 10 whatever T): D_t = M M^T / d + 2.5 I,
    |S_t| ~ 0.8 in spectral norm, so block Gershgorin keeps the smallest eigenvalue near 1.
    (The L L^T generator above becomes exponentially ill-conditioned in T and is kept for tiny T only.)
    """
    M = rng.normal(size=batch + (T, d, d))
    diag = M @ np.swapaxes(M, -1, -2) / d + 2.5 * np.eye(d)
    sub = 0.4 * rng.normal(size=batch + (max(T - 1, 0), d, d)) / np.sqrt(d)
    return diag, (sub if T > 1 else None)


def random_ssm_params(rng, batch, T, d, scale_A=0.6):
    """Random stable SSM parameters (mu0, cholP0, A, b, cholQ)."""
    A = scale_A * rng.normal(size=batch + (T - 1, d, d)) / np.sqrt(d)
    b = rng.normal(size=batch + (T - 1, d))
    idx = np.arange(d)
    cholQ = np.tril(0.3 * rng.normal(size=batch + (T - 1, d, d)))
    cholQ[..., idx, idx] = np.abs(cholQ[..., idx, idx]) + 0.5
    cholP0 = np.tril(0.3 * rng.normal(size=batch + (d, d)))
    cholP0[..., idx, idx] = np.abs(cholP0[..., idx, idx]) + 0.5
    mu0 = rng.normal(size=batch + (d,))
    return mu0, cholP0, A, b, cholQ


def assert_close(actual, desired, rtol=1e-6, scale_atol=1e-8):
    """Element-wise rtol plus an absolute floor tied to the tensor's own magnitude (fp64 parity; the
    north-star bound is 1e-5 relative)."""
    desired = np.asarray(desired)
    atol = scale_atol * max(1.0, float(np.max(np.abs(desired))) if desired.size else 1.0)
    np.testing.assert_allclose(actual, desired, rtol=rtol, atol=atol)


# ---- inputs of the quadrature-kernel tests (tests/test_host_quad.py, tests/test_gpu_quad.py) ------------------------------------------
def random_quad_path(rng, B, T, d, min_mean=None):
    """Marginals mu [B, T, d], Sig [B, T, d, d] and subsequent covariances Sub [B, T-1, d, d] of B random stable SSMs
    (oracle.np_ssm), rescaled so that the largest marginal standard deviation is 0.6 and, with `min_mean`, the means shifted so that
    the smallest is that.  Asserts what the quadrature tests rely on: standard deviations within [0.2, 0.6] and every eigenvalue of
    S_t and of Qq_t = S_{t+1} - C_t S_t^{-1} C_t^T above 0.02."""
    from oracle import np_ssm
    mu0, cholP0, A, off, cholQ = random_ssm_params(rng, (B,), T, d, scale_A=0.35)
    idx = np.arange(d)
    for c in (cholP0, cholQ):       # process noise of similar size everywhere, so that the standard deviations stay within a factor 3
        c *= 0.8
        c[..., idx, idx] = 0.8 + 0.2 * rng.random(c.shape[:-1])
    prm = (mu0, cholP0, A, off, cholQ)
    mus, covs, subs = [], [], []
    for b in range(B):
        ssm = np_ssm.StateSpaceModel(*[p[b] for p in prm])
        mu, cov = ssm.marginals
        mus.append(mu); covs.append(cov); subs.append(ssm.subsequent_covariances(cov))
    mu, cov, sub = np.stack(mus), np.stack(covs), np.stack(subs)
    s = 0.6 / np.sqrt(np.max(np.einsum("...ii->...i", cov)))
    mu, cov, sub = s * mu, s * s * cov, s * s * sub
    if min_mean is not None:
        mu = mu + (min_mean - mu.min())
    cov = 0.5 * (cov + np.swapaxes(cov, -1, -2))
    sd = np.sqrt(np.einsum("...ii->...i", cov))
    assert sd.min() >= 0.2 and sd.max() <= 0.6 + 1e-12, (sd.min(), sd.max())
    Qq = cov[:, 1:] - sub @ np.linalg.solve(cov[:, :-1], np.swapaxes(sub, -1, -2))
    assert np.linalg.eigvalsh(cov).min() > 0.02 and np.linalg.eigvalsh(0.5 * (Qq + np.swapaxes(Qq, -1, -2))).min() > 0.02
    return mu, cov, sub


QUAD_DT = 0.05
QUAD_Q = {1: np.array([[0.7]]), 2: np.array([[0.5, 0.12], [0.12, 0.4]]), 3: np.array([[0.8, -0.2, 0.1], [-0.2, 0.6, 0.15], [0.1, 0.15, 0.7]])}
QUAD_P0 = {1: np.array([[0.6]]), 2: np.array([[0.7, 0.1], [0.1, 0.5]]), 3: np.array([[0.7, 0.1, -0.15], [0.1, 0.5, 0.2], [-0.15, 0.2, 0.6]])}
QUAD_MU0 = np.array([0.1, -0.2, 0.05])
QUAD_KL_CASES = {10: (2, 0), 11: (3, 4), 12: (3, 0), 13: (3, 0), 14: (3, 0), 15: (3, 0)}       # kind: (d, nh)


def quad_theta(kind, nh=0):
    """Drift parameters of the quadrature kernels' kinds 10 .. 15 as include/mfgm.h lays them out (the network's from a generator of
    their own)."""
    if kind == 11:
        r = np.random.default_rng(1234 + nh)
        return np.concatenate([r.normal(size=nh), 0.3 * r.normal(size=nh), r.normal(size=nh) / np.sqrt(nh), [0.2]])
    return np.array({10: [1.3, 0.9], 12: [1.4, 2.0], 13: [1.3, 0.0], 14: [0.4, 0.0], 15: [1.5, 0.0]}[kind])


def quad_kl_case(kind):
    """The KL parity case of one drift kind, the same for the host and the GPU tests: B = 3 chains of T = 5 nodes, full q and P0, from
    a generator seeded by the kind.  Kind 15: the means are shifted to 8 and above -- beyond 4, because the outermost nodes of the
    20-point rule lie up to sqrt(2) * 5.39 standard deviations per dimension from the mean and none may come near the kink at 0."""
    d, nh = QUAD_KL_CASES[kind]
    mu, cov, sub = random_quad_path(np.random.default_rng(71892305 + kind), 3, 5, d, min_mean=8.0 if kind == 15 else None)
    return dict(kind=kind, d=d, nh=nh, th=quad_theta(kind, nh), dt=QUAD_DT, q=QUAD_Q[d], mu0=QUAD_MU0[:d], P0=QUAD_P0[d], mu=mu, cov=cov,
                sub=sub)
