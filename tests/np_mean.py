"""
NumPy restatement, in np.longdouble, of the impulse and step mean functions (markovflow/mean_function.py `ImpulseMeanFunction`,
`StepMeanFunction`): the sequential recurrence  c_k = A(t_k - t_k-1) c_k-1 + rhs_k,  c_-1 = 0,  and the evaluation
mu(t) = shift_k + A(t - t_k) c_k  with  k = #{i : t_i < t} - 1  (zero when no action lies before t), on the transition closed forms of
the NumPy kernels the tests already have (oracle/np_kernels.py, tests/np_kernels_ext.py).  Every result comes with the absolute-value
recurrence  sum |A| |c| + |rhs|  beside it: the scale the errors of the device kernels are measured against.
"""
import numpy as np

from oracle import np_kernels
from tests import np_kernels_ext as E

LD = np.longdouble


def tree(d, m, x):
    """The kernel tree of state dimension d = 1 .. 8 the mean-function tests use, from the Matern module m and the seasonal module x
    (vidp_amd.kernels twice, or np_kernels and np_kernels_ext)."""
    P, S, HO = x.Product, m.Sum, x.HarmonicOscillator
    return {
        1: lambda: m.Matern12(0.7, 1.1),
        2: lambda: m.Matern32(1.3, 0.8),
        3: lambda: m.Matern52(0.9, 1.2),
        4: lambda: S([m.Matern32(1.3, 0.8), m.Matern32(0.6, 1.5)]),
        5: lambda: S([m.Matern52(0.9, 1.2), P([m.Matern12(0.7, 1.1), HO(0.9, 2.0)])]),
        6: lambda: P([m.Matern32(1.3, 0.8), m.Matern52(0.9, 1.2)]),
        7: lambda: S([m.Matern52(0.9, 1.2), m.Matern32(1.3, 0.8), m.Matern32(0.6, 1.5)]),
        8: lambda: P([m.Matern32(1.3, 0.8), HO(0.9, 2.0), HO(1.4, 3.1)]),
    }[d]()


def _block_diag(mats):
    batch = np.broadcast_shapes(*[a.shape[:-2] for a in mats])
    n = sum(a.shape[-1] for a in mats)
    out = np.zeros(batch + (n, n), dtype=LD)
    i = 0
    for a in mats:
        k = a.shape[-1]
        out[..., i:i + k, i:i + k] = a
        i += k
    return out


def transitions(kernel, dt):
    """A(dt) [..., d, d] in long double: the leaves' closed forms, Kronecker products under Product, blocks under Sum."""
    dt = np.asarray(dt, dtype=LD)
    if isinstance(kernel, np_kernels.Sum):
        return _block_diag([transitions(k, dt) for k in kernel.kernels])
    if isinstance(kernel, E.Product):
        out = transitions(kernel.kernels[0], dt)
        for k in kernel.kernels[1:]:
            out = E.kron(out, transitions(k, dt))
        return out
    if isinstance(kernel, np_kernels.Matern12):
        # (the package hands the device rate = 1 / lengthscale)
        return np.exp(-dt * LD(1.0 / kernel.lengthscale))[..., None, None]
    A = np.asarray(kernel.state_transitions(dt))
    assert A.dtype == LD or isinstance(kernel, E.Constant)
    return A.astype(LD)


def generator(kernel):
    """G with A(dt) = expm(G dt): the feedback matrix of the leaves, blocks under Sum, the Kronecker SUM under Product (whose
    feedback_matrix() is the reference's Kronecker product)."""
    if isinstance(kernel, np_kernels.Sum):
        return _block_diag([generator(k) for k in kernel.kernels])
    if isinstance(kernel, E.Product):
        G = generator(kernel.kernels[0])
        for k in kernel.kernels[1:]:
            g = generator(k)
            G = E.kron(G, np.eye(g.shape[-1], dtype=LD)) + E.kron(np.eye(G.shape[-1], dtype=LD), g)
        return G
    return np.asarray(kernel.feedback_matrix(), dtype=LD)


def solve(G, rhs):
    """G^-1 rhs for rhs [..., d] by Gaussian elimination with partial pivoting in long double (LAPACK has none)."""
    G = np.array(G, dtype=LD)
    d = G.shape[0]
    x = np.array(rhs, dtype=LD).reshape(-1, d).T.copy()
    for i in range(d):
        p = i + int(np.argmax(np.abs(G[i:, i])))
        if G[p, i] == 0:
            raise ZeroDivisionError("singular matrix")
        G[[i, p]], x[[i, p]] = G[[p, i]], x[[p, i]]
        for r in range(i + 1, d):
            f = G[r, i] / G[i, i]
            G[r, i:] -= f * G[i, i:]
            x[r] -= f * x[i]
    for i in range(d - 1, -1, -1):
        x[i] = (x[i] - G[i, i + 1:] @ x[i + 1:]) / G[i, i]
    return x.T.reshape(np.shape(rhs))


def step_rhs(kernel, u):
    """(rhs, shift) [K, d] of the step perturbations u [K, d]: a_k = -G^-1 u_k, shift = a, rhs_k = a_k-1 - a_k with a_-1 = 0."""
    a = -solve(generator(kernel), u)
    rhs = -a.copy()
    rhs[1:] += a[:-1]
    return rhs, a


def coefficients(kernel, times, rhs):
    """(c, scale) [K, d]: the sequential recurrence over one chain and its absolute-value twin."""
    times = np.asarray(times, dtype=np.float64)
    rhs = np.asarray(rhs, dtype=LD)
    K, d = rhs.shape
    c, s = np.zeros((K, d), dtype=LD), np.zeros((K, d), dtype=LD)
    c[0], s[0] = rhs[0], np.abs(rhs[0])
    A = transitions(kernel, times[1:].astype(LD) - times[:-1].astype(LD))          # [K - 1, d, d]
    for k in range(1, K):
        c[k] = A[k - 1] @ c[k - 1] + rhs[k]
        s[k] = np.abs(A[k - 1]) @ s[k - 1] + np.abs(rhs[k])
    return c, s


def evaluate(kernel, times, coef, scale, shift, tq):
    """(mu, mu_scale) [N, d] at the unordered query points tq [N]."""
    times = np.asarray(times, dtype=np.float64)
    tq = np.asarray(tq, dtype=np.float64)
    d = coef.shape[-1]
    mu, ms = np.zeros((len(tq), d), dtype=LD), np.zeros((len(tq), d), dtype=LD)
    j = np.searchsorted(times, tq, side="left")          # #{i : t_i < t}
    seen = np.nonzero(j > 0)[0]
    if seen.size:
        k = j[seen] - 1
        A = transitions(kernel, tq[seen].astype(LD) - times[k].astype(LD))         # [n, d, d]
        mu[seen] = np.einsum("nij,nj->ni", A, coef[k])
        ms[seen] = np.einsum("nij,nj->ni", np.abs(A), scale[k])
        if shift is not None:
            sh = np.asarray(shift, dtype=LD)[k]
            mu[seen] += sh
            ms[seen] += np.abs(sh)
    return mu, ms


def emission(kernel):
    return np.asarray(kernel.emission_vector(), dtype=LD).reshape(-1)


def mean(kernel, kind, times, u, tq):
    """The whole mean function of one chain from the perturbations u [K, d]: dict(coef, scale, shift, mu, mu_scale, f, f_scale)."""
    u = np.asarray(u, dtype=LD)
    rhs, shift = (u, None) if kind == "impulse" else step_rhs(kernel, u)
    c, s = coefficients(kernel, times, rhs)
    mu, ms = evaluate(kernel, times, c, s, shift, tq)
    h = emission(kernel)
    return dict(coef=c, scale=s, shift=shift, mu=mu, mu_scale=ms, f=mu @ h, f_scale=ms @ np.abs(h))
