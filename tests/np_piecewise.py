"""
NumPy restatement of the piecewise-stationary kernel (vidp_amd.kernels.PiecewiseKernel, include/mfgm.h `mfgm_packed_piecewise_ssm`),
written from its contract:

    region       r(t) = #{c_k <= t}: a point on a change point belongs to the region after it
    transition   t_k -> t_k+1 takes child r(t_k) -- the region of its LEFT end, also when it crosses a change point:
                 A = A_r(dt), Q = Pinf_r - A Pinf_r A^T + jitter, b = (I - A) m_r
    first state  mean ZERO, covariance Pinf_r(t_0) + jitter

A plain loop over the transitions; each child's (A, Q, b, Pinf) comes from the NumPy kernels of oracle.np_kernels and
tests/np_kernels_ext.  Plus what the model tests need on top of it: the dense prior mean and covariance of f on a grid, time-aware
conditionals and a sparse CVI model that uses them (oracle.np_conditionals passes no transition times).
"""
import numpy as np

from oracle import np_conditionals as npc
from oracle import np_kernels
from oracle.np_ssm import state_space_model_from_covariances
from tests import np_kernels_ext as E


class PiecewiseKernel:
    def __init__(self, kernels, change_points, jitter=0.0):
        self.kernels = list(kernels)
        self.change_points = np.asarray(change_points, dtype=np.float64).reshape(-1)
        assert len(self.kernels) == self.change_points.size + 1
        self.jitter = float(jitter)
        self.state_dim = self.kernels[0].state_dim

    def region(self, t):
        """#{c_k <= t} for every entry of t."""
        t = np.asarray(t, dtype=np.float64)
        return np.sum(self.change_points[(None,) * t.ndim] <= t[..., None], axis=-1)

    def steady_state_covariance_at(self, t):
        return np.stack([k.steady_state_covariance() for k in self.kernels])[self.region(t)]

    def feedback_matrix_at(self, t):
        return np.stack([k.feedback_matrix() for k in self.kernels])[self.region(t)]

    def state_mean_at(self, t):
        return np.stack([k.state_mean for k in self.kernels])[self.region(t)]

    def transition(self, t_left, dt):
        """(A, Q, b) of ONE transition that starts at t_left and lasts dt."""
        k = self.kernels[int(self.region(t_left))]
        A, Q = k.transition_statistics(np.asarray(dt, dtype=np.float64))
        return A, Q + self.jitter * np.eye(self.state_dim), k.state_offsets(np.asarray(dt, dtype=np.float64))

    def transition_statistics_at(self, t_left, dt):
        """(A, Q, b) for arrays of left ends and gaps of one shape: the loop over the transitions."""
        t_left, dt = np.broadcast_arrays(np.asarray(t_left, dtype=np.float64), np.asarray(dt, dtype=np.float64))
        d = self.state_dim
        A, Q, b = np.zeros(dt.shape + (d, d)), np.zeros(dt.shape + (d, d)), np.zeros(dt.shape + (d,))
        for i in np.ndindex(dt.shape):
            A[i], Q[i], b[i] = self.transition(t_left[i], dt[i])
        return A, Q, b

    def initial_covariance_at(self, t0):
        return self.steady_state_covariance_at(t0) + self.jitter * np.eye(self.state_dim)

    def ssm_parameters(self, t):
        """(mu0, P0, A, b, Q) at the sorted points t [..., T]."""
        t = np.asarray(t, dtype=np.float64)
        A, Q, b = self.transition_statistics_at(t[..., :-1], np.diff(t, axis=-1))
        return np.zeros(t.shape[:-1] + (self.state_dim,)), self.initial_covariance_at(t[..., 0]), A, b, Q

    def state_space_model(self, t):
        mu0, P0, A, b, Q = self.ssm_parameters(t)
        return state_space_model_from_covariances(mu0, P0, A, b, Q)

    def emission_vector(self):
        return self.kernels[0].emission_vector()

    def emission_matrix(self, t):
        return np.broadcast_to(self.emission_vector(), np.shape(t) + (1, self.state_dim)).copy()


def f_covariance(kernel, t):
    """Dense covariance of f = H s on the sorted points t [T] under the piecewise SSM."""
    _, P0, A, _, Q = kernel.ssm_parameters(t)
    return E.f_covariance(A, Q, P0, kernel.emission_vector())


def f_mean(kernel, t):
    """Prior mean of f on the sorted points t [T]: m_0 = 0, m_k+1 = A_k m_k + b_k."""
    mu0, _, A, b, _ = kernel.ssm_parameters(t)
    m = [mu0]
    for k in range(A.shape[0]):
        m.append(A[k] @ m[-1] + b[k])
    return np.stack(m) @ kernel.emission_vector()[0]


def stitched_parameters(kernels, grids):
    """(P0, A, Q) of the chain that follows kernels[i] (stationary NumPy kernels) on grids[i], each grid starting where the one before
    ends: the first grid's stationary start, then every grid's own transitions."""
    A = np.concatenate([k.transition_statistics(np.diff(g))[0] for k, g in zip(kernels, grids)])
    Q = np.concatenate([k.transition_statistics(np.diff(g))[1] for k, g in zip(kernels, grids)])
    return kernels[0].initial_covariance(), A, Q


def marginal_covariances(P0, A, Q):
    S = [P0]
    for k in range(A.shape[0]):
        S.append(A[k] @ S[-1] @ A[k].T + Q[k])
    return np.stack(S)


# ---- conditionals with transition times (markovflow/conditionals.py:207-256 passes (minus, t - minus) and (t, plus - t)) --------------
def conditional_statistics(new_t, train_t, kernel):
    idx = np.searchsorted(train_t, new_t, side="left")
    aug = np.concatenate([[-npc.APPROX_INF], train_t, [npc.APPROX_INF]])
    A_mt, Q_mt, _ = kernel.transition_statistics_at(aug[idx], new_t - aug[idx])
    A_tp, Q_tp, _ = kernel.transition_statistics_at(new_t, aug[idx + 1] - new_t)
    D, Ec, T = npc.cond_stats_from_transitions(A_mt, Q_mt, A_tp, Q_tp)
    return np.concatenate([D, Ec], axis=-1), T, idx


def predict_f(ssm, kernel, cond_t, new_t):
    jm, jc = npc.pairwise_marginals(ssm, np.zeros(kernel.state_dim), kernel.initial_covariance_at(cond_t[0]))
    P, T, idx = conditional_statistics(new_t, cond_t, kernel)
    m, S = (P @ jm[idx][..., None])[..., 0], T + P @ jc[idx] @ np.swapaxes(P, -1, -2)
    h = kernel.emission_vector()[0]
    return (m @ h)[:, None], np.einsum("i,nij,j->n", h, S, h)[:, None]


class SparseCVIGaussianProcess(npc.SparseCVIGaussianProcess):
    """oracle.np_conditionals.SparseCVIGaussianProcess with the time-aware conditionals above."""

    def update_sites(self, t, y):
        mu, var = predict_f(self.dist_q, self.kernel, self.z, t)
        g1, g2 = self.lik.grads_expectation(mu, var, y)
        P, _, idx = conditional_statistics(t, self.z, self.kernel)
        HP = self.kernel.emission_vector()[None] @ P
        bp1 = np.sum(HP * g1[..., None], axis=-2)
        bp2 = np.sum(g2[..., None, None] * HP[..., None] * HP[..., None, :], axis=-3)
        s1, s2 = np.zeros_like(self.nat1), np.zeros_like(self.nat2)
        np.add.at(s1, idx, bp1)
        np.add.at(s2, idx, bp2)
        self.nat1 = (1 - self.lr) * self.nat1 + self.lr * s1
        self.nat2 = (1 - self.lr) * self.nat2 + self.lr * s2

    def classic_elbo(self, t, y):
        q = self.dist_q
        mu, var = predict_f(q, self.kernel, self.z, t)
        return np.sum(self.lik.variational_expectations(mu, var, y)) - np.sum(q.kl_divergence(self.dist_p))


# ---- the cases the host and the GPU tests share ---------------------------------------------------------------------------------------
def stitched_case():
    """The reference's two-region case: Matern32 (l, v) = (1, 1) before and (2, 2) after the change point -1e-5, on
    linspace(-1, 0, 5) and linspace(0, 1, 5) joined at 0."""
    ks = [np_kernels.Matern32(1.0, 1.0), np_kernels.Matern32(2.0, 2.0)]
    xs = [np.linspace(-1.0, 0.0, 5), np.linspace(0.0, 1.0, 5)]
    return ks, xs, np.concatenate([xs[0], xs[1][1:]])


def gpr_case(rng):
    """Test 5 of tests/test_gpu_piecewise.py: T = 60, Matern32, 3 regions, gaps >= 0.03."""
    t = np.cumsum(0.03 + rng.exponential(0.07, size=60))
    cp = [t[17], 0.5 * (t[40] + t[41])]
    prm = [(0.6, 1.0), (1.5, 0.4), (0.3, 2.0)]
    y = np.sin(2.0 * t)[:, None] + 0.3 * rng.normal(size=(60, 1))
    return t, y, cp, prm, 0.2


def dense_logml(Kd, resid):
    L = np.linalg.cholesky(Kd)
    a = np.linalg.solve(L, resid)
    return -0.5 * a @ a - np.log(np.diag(L)).sum() - 0.5 * resid.size * np.log(2 * np.pi)


def predict_case(rng):
    """Test 6 of tests/test_gpu_piecewise.py: 40 training points, 3 regions with the change points ON training points, 25 new unsorted
    times before, inside every region and after."""
    t = np.cumsum(0.05 + rng.exponential(0.1, size=40))
    cp = [t[12], t[27]]
    prm = [(0.6, 1.0), (1.5, 0.4), (0.3, 2.0)]
    y = np.cos(1.5 * t)[:, None] + 0.2 * rng.normal(size=(40, 1))
    tn = np.concatenate([t[0] - rng.uniform(0.1, 1.0, size=3), t[-1] + rng.uniform(0.1, 1.0, size=3), rng.uniform(t[0], t[12], size=6),
                         rng.uniform(t[12], t[27], size=7), rng.uniform(t[27], t[-1], size=6)])
    return t, y, cp, prm, 0.1, rng.permutation(tn)


def dense_predict(pk, t, y, noise, tn):
    """Dense conditioning of the piecewise SSM built on the union grid."""
    u = np.concatenate([t, tn])
    order = np.argsort(u, kind="stable")
    Ku = f_covariance(pk, u[order])
    inv = np.argsort(order)
    Ku = Ku[np.ix_(inv, inv)]
    n = t.size
    Kd, Ks = Ku[:n, :n] + noise * np.eye(n), Ku[n:, :n]
    return Ks @ np.linalg.solve(Kd, y[:, 0]), np.diag(Ku[n:, n:]) - np.einsum("ij,ji->i", Ks, np.linalg.solve(Kd, Ks.T))
