"""
Spatial kernels on R^p for the spatio-temporal models (the reference hands gpflow.kernels.SquaredExponential / Matern12 / Matern32 /
Matern52 to SparseSpatioTemporalKernel, spatio_temporal_variational.py:45-106): stationary kernels of the scaled distance
r = |(x - x') / lengthscales| in plain torch -- they are evaluated once per data set, at the spatial inducing points and between
them and the data.  Named apart from the temporal (state-space) kernels of vidp_amd.kernels: space_kernels.Matern32 is a function
of space, kernels.Matern32 a Markov process in time.
"""
import math

import torch


class _Stationary:
    def __init__(self, lengthscales=1.0, variance=1.0):
        ls = torch.as_tensor(lengthscales, dtype=torch.float64)
        if ls.dim() > 1 or bool((ls <= 0).any()) or float(variance) <= 0.0:
            raise ValueError("lengthscales (a scalar or [p]) and variance must be positive")
        self.lengthscales, self.variance = ls, float(variance)

    def _scaled(self, X):
        X = torch.as_tensor(X, dtype=torch.float64)
        ls = self.lengthscales.to(X.device)
        if ls.dim() == 1 and ls.shape[0] != X.shape[-1]:
            raise ValueError(f"{ls.shape[0]} lengthscales for inputs of dimension {X.shape[-1]}")
        return X / ls

    def _r2(self, X, X2):
        A = self._scaled(X)
        B = A if X2 is None else self._scaled(X2)
        diff = A[..., :, None, :] - B[..., None, :, :]
        return (diff * diff).sum(-1)

    def _k(self, r2):
        raise NotImplementedError

    def K(self, X, X2=None):
        """[..., N, N2] covariance between the rows of X [..., N, p] and of X2 (X when None)."""
        return self._k(self._r2(X, X2))

    def K_diag(self, X):
        """[..., N]: k(x, x) = variance."""
        X = torch.as_tensor(X, dtype=torch.float64)
        return torch.full(tuple(X.shape[:-1]), self.variance, dtype=torch.float64, device=X.device)

    __call__ = K


class SquaredExponential(_Stationary):
    """variance exp(-r^2 / 2)."""

    def _k(self, r2):
        return self.variance * torch.exp(-0.5 * r2)


class Matern12(_Stationary):
    """variance exp(-r)."""

    def _k(self, r2):
        return self.variance * torch.exp(-torch.sqrt(r2))


class Matern32(_Stationary):
    """variance (1 + sqrt(3) r) exp(-sqrt(3) r)."""

    def _k(self, r2):
        s = math.sqrt(3.0) * torch.sqrt(r2)
        return self.variance * (1.0 + s) * torch.exp(-s)


class Matern52(_Stationary):
    """variance (1 + sqrt(5) r + 5 r^2 / 3) exp(-sqrt(5) r)."""

    def _k(self, r2):
        s = math.sqrt(5.0) * torch.sqrt(r2)
        return self.variance * (1.0 + s + (5.0 / 3.0) * r2) * torch.exp(-s)
