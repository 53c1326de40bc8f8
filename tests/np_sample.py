"""NumPy restatement of the sampling contract of include/mfgm.h (mfgm_packed_sample): block Cholesky Lambda = L L^T, y = L^{-1} r,
eps[n, b, t] = z[i = n, k = b T + t] of the normal stream with tag s, and x = L^{-T} (y + eps)."""
import numpy as np

from oracle import np_btd
from tests.np_sim import normals


def eps(seed, s, S, B, T, d):
    """[S, B, T, d]: the noise of samples 0..S-1 of B chains of T nodes."""
    return normals(seed, s, np.arange(S), np.arange(B * T), d).reshape(S, B, T, d)


def sample(diag, sub, r, seed, s, S):
    """(x [S, B, T, d], eps, (Ld, Ls), y) for the precision blocks (diag [B, T, d, d], sub [B, T-1, d, d] or None) and rhs r [B, T, d]."""
    B, T, d = np.asarray(r).shape
    Ld, Ls = np_btd.cholesky(diag, sub)
    y = np_btd.solve(Ld, Ls, r)
    e = eps(seed, s, S, B, T, d)
    x = np_btd.solve(Ld[None], None if Ls is None else Ls[None], y[None] + e, transpose_left=True)
    return x, e, (Ld, Ls), y
