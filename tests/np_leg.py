"""
NumPy restatement of the latent exponentially generated kernel (markovflow/kernels/latent_exp_generated.py
`LatentExponentiallyGenerated`) as a subclass of oracle.np_kernels.StationaryKernel, so that the oracle models
(np_models.gpr_log_likelihood, np_models.CVIGaussianProcess, np_conditionals) take it: F = -(N N^T + R - R^T) / 2, Pinf = I,
A = expm(F dt), Q = Pinf - A Pinf A^T + jitter (the base class's rule).  The matrix exponential is an np.longdouble, degree-30
scaling-and-squaring Taylor series rounded to fp64 (no SciPy).  Plus an independent known answer, the dense covariance
k(tau) = h expm(F |tau|) h^T, and a restatement in fp64 of the arithmetic of the device function leg_expm (csrc/mfgm_leg_ssm.h).
"""
import numpy as np

from oracle import np_kernels


def expm_ld(X, degree=30):
    """expm of the trailing square matrices of X (any batch shape) in np.longdouble: scaled so that |X|_1 / 2^s <= 1/2, Taylor
    polynomial of the given degree in Horner form, s squarings; returned in longdouble."""
    X = np.asarray(X, dtype=np.longdouble)
    d = X.shape[-1]
    eye = np.eye(d, dtype=np.longdouble)
    norm = np.abs(X).sum(axis=-2).max(axis=-1) if X.size else np.zeros(X.shape[:-2], dtype=np.longdouble)
    s = np.where(norm > 0.5, np.ceil(np.log2(np.maximum(norm.astype(np.float64), 0.5) / 0.5)), 0.0).astype(int)
    Xs = X / (np.longdouble(2.0) ** s)[..., None, None]
    P = np.broadcast_to(eye, X.shape).copy()
    for k in range(degree, 0, -1):
        P = eye + (Xs @ P) / np.longdouble(k)
    for r in range(int(s.max()) if s.size else 0):
        P = np.where((s > r)[..., None, None], P @ P, P)
    return P


def expm(X):
    """expm_ld rounded to fp64."""
    return expm_ld(X).astype(np.float64)


def expm_eig(X):
    """expm through the eigendecomposition V exp(Lambda) V^-1 (complex, fp64): an independent route for diagonalisable X."""
    w, V = np.linalg.eig(np.asarray(X, dtype=np.float64))
    return np.real((V * np.exp(w)[..., None, :]) @ np.linalg.inv(V))


def device_expm(F, dt, max_degree=18, truncation=1e-18):
    """The arithmetic of leg_expm for one gap, in fp64 (products by np.matmul instead of fma chains): theta = |F|_1 dt, s = 0 for
    theta <= 1/2 else ilogb(theta) + 2, the smallest degree m whose first dropped term (theta / 2^s)^(m+1) / (m+1)! is below the
    truncation, P = I + (h / m) F, P <- I + (h / k) F P for k = m-1 .. 1 with h = dt / 2^s, s squarings.  Returns (A, m, s)."""
    F = np.asarray(F, dtype=np.float64)
    d = F.shape[-1]
    eye = np.eye(d)
    theta = np.abs(F).sum(axis=0).max() * dt
    s = 0
    if theta > 0.5:
        s = int(np.floor(np.log2(theta))) + 2
    h, th = np.ldexp(dt, -s), np.ldexp(theta, -s)
    m, term = 1, th
    while m < max_degree:
        term *= th / (m + 1)
        if not term > truncation:
            break
        m += 1
    P = eye + (h / m) * F
    for k in range(m - 1, 0, -1):
        P = eye + (h / k) * (F @ P)
    for _ in range(s):
        P = P @ P
    return P, m, s


class LatentExponentiallyGenerated(np_kernels.StationaryKernel):
    """latent_exp_generated.py:28-142, single output: emission row e_1, or `emission` [d] (the LEG paper's B)."""

    def __init__(self, N, R, jitter=0.0, emission=None):
        super().__init__(jitter)
        self.N, self.R = np.array(N, dtype=np.float64), np.array(R, dtype=np.float64)
        self.state_dim = self.N.shape[0]
        self.emission = None if emission is None else np.array(emission, dtype=np.float64).reshape(-1)

    def feedback_matrix(self):
        return -0.5 * (self.N @ self.N.T + self.R - self.R.T)

    def steady_state_covariance(self):
        return np.eye(self.state_dim)

    def state_transitions(self, time_deltas):
        dt = np.asarray(time_deltas, dtype=np.float64)
        return expm(self.feedback_matrix() * dt[..., None, None])

    def emission_vector(self):
        if self.emission is None:
            return super().emission_vector()
        return self.emission[None].copy()


def dense_k(kernel, tau):
    """k(tau) = h expm(F |tau|) h^T of a LatentExponentiallyGenerated (Pinf = I), any shape of tau."""
    r = np.abs(np.asarray(tau, dtype=np.float64))
    h = kernel.emission_vector()[0]
    A = expm(kernel.feedback_matrix() * r[..., None, None])
    return np.einsum("i,...ij,j->...", h, A, h)
