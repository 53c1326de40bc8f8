"""
NumPy restatement of the seasonal SDE kernels (markovflow/kernels/periodic.py `HarmonicOscillator`, kernels/constant.py `Constant`,
kernels/sde_kernel.py `Product`) as subclasses of oracle.np_kernels.StationaryKernel, following the reference formulas literally
(Q = Pinf - A Pinf A^T + jitter, Constant's Q = 0 + jitter), so that the oracle models (np_models.gpr_log_likelihood,
np_models.CVIGaussianProcess, np_conditionals) take them.  Plus an independent known answer: the dense covariance function k(tau) of
any Matern / OU / Constant / HarmonicOscillator / Product / Sum tree in closed form.
"""
import numpy as np

from oracle import np_kernels


def kron(X, Y):
    """Kronecker product of the trailing square matrices, batch dimensions broadcast."""
    a, b = X.shape[-1], Y.shape[-1]
    out = X[..., :, None, :, None] * Y[..., None, :, None, :]
    return out.reshape(out.shape[:-4] + (a * b, a * b))


class HarmonicOscillator(np_kernels.StationaryKernel):
    """periodic.py:27-203."""
    state_dim = 2

    def __init__(self, variance, period, jitter=0.0):
        super().__init__(jitter)
        self.variance, self.period = float(variance), float(period)
        self.lam = 2.0 * np.pi / self.period

    def state_transitions(self, time_deltas):
        x = np.asarray(time_deltas)[..., None, None] * self.lam
        c, s = np.cos(x), np.sin(x)
        return np.concatenate([np.concatenate([c, -s], axis=-1), np.concatenate([s, c], axis=-1)], axis=-2)

    def feedback_matrix(self):
        return np.array([[0.0, -self.lam], [self.lam, 0.0]])

    def steady_state_covariance(self):
        return self.variance * np.eye(2)


class Constant(np_kernels.StationaryKernel):
    """constant.py:28-153 (transition_statistics is overridden there: Q = 0 + jitter)."""
    state_dim = 1

    def __init__(self, variance, jitter=0.0):
        super().__init__(jitter)
        self.variance = float(variance)

    def state_transitions(self, time_deltas):
        return np.ones(np.shape(time_deltas) + (1, 1))

    def transition_statistics(self, time_deltas):
        A = self.state_transitions(time_deltas)
        return A, np.zeros_like(A) + self.jitter * np.eye(1)

    def feedback_matrix(self):
        return np.zeros((1, 1))

    def steady_state_covariance(self):
        return np.array([[self.variance]])


class Product(np_kernels.StationaryKernel):
    """sde_kernel.py:691-826: Kronecker products of the children's A, Pinf, F and H; Q from the inherited transition_statistics."""

    def __init__(self, kernels, jitter=0.0):
        super().__init__(jitter)
        self.kernels = list(kernels)
        self.state_dim = int(np.prod([k.state_dim for k in self.kernels]))

    def _kron_all(self, mats):
        out = mats[0]
        for m in mats[1:]:
            out = kron(out, m)
        return out

    def state_transitions(self, time_deltas):
        return self._kron_all([k.state_transitions(time_deltas) for k in self.kernels])

    def feedback_matrix(self):
        return self._kron_all([k.feedback_matrix() for k in self.kernels])

    def steady_state_covariance(self):
        return self._kron_all([k.steady_state_covariance() for k in self.kernels])

    def emission_vector(self):
        h = self.kernels[0].emission_vector()
        for k in self.kernels[1:]:
            h = np.kron(h, k.emission_vector())
        return h


def dense_k(kernel, tau):
    """k(tau) in closed form for a tree of np_kernels / np_kernels_ext kernels."""
    r = np.abs(np.asarray(tau, dtype=np.float64))
    if isinstance(kernel, HarmonicOscillator):
        return kernel.variance * np.cos(2.0 * np.pi * r / kernel.period)
    if isinstance(kernel, Constant):
        return kernel.variance * np.ones_like(r)
    if isinstance(kernel, Product):
        out = np.ones_like(r)
        for k in kernel.kernels:
            out = out * dense_k(k, r)
        return out
    if isinstance(kernel, np_kernels.Sum):
        return sum(dense_k(k, r) for k in kernel.kernels)
    if isinstance(kernel, np_kernels.Matern12):
        return kernel.variance * np.exp(-r / kernel.lengthscale)
    if isinstance(kernel, np_kernels.OrnsteinUhlenbeck):
        return kernel.diffusion / (2.0 * kernel.decay) * np.exp(-kernel.decay * r)
    if isinstance(kernel, np_kernels.Matern32):
        x = np.sqrt(3.0) * r / kernel.lengthscale
        return kernel.variance * (1.0 + x) * np.exp(-x)
    if isinstance(kernel, np_kernels.Matern52):
        x = np.sqrt(5.0) * r / kernel.lengthscale
        return kernel.variance * (1.0 + x + x * x / 3.0) * np.exp(-x)
    raise TypeError(type(kernel))


def f_covariance(A, Q, P0, H):
    """H Sigma(t_i, t_j) H^T of a state-space prior (A, Q [n-1, d, d], P0 [d, d], H [1, d]) as a dense n x n matrix: Sigma_ii by the
    forward recursion, Sigma_ij = A(t_i <- t_j) Sigma_jj for i > j."""
    n = A.shape[0] + 1
    S = [P0]
    for k in range(n - 1):
        S.append(A[k] @ S[-1] @ A[k].T + Q[k])
    K = np.zeros((n, n))
    for j in range(n):
        C = S[j]
        K[j, j] = (H @ C @ H.T)[0, 0]
        for i in range(j + 1, n):
            C = A[i - 1] @ C
            K[i, j] = K[j, i] = (H @ C @ H.T)[0, 0]
    return K


def ssm_f_covariance(kernel, t):
    """f_covariance of an np_kernels / np_kernels_ext kernel's state-space prior on the sorted points t."""
    A, Q = kernel.transition_statistics(np.diff(np.asarray(t, dtype=np.float64)))
    return f_covariance(A, Q, kernel.initial_covariance(), kernel.emission_vector())
