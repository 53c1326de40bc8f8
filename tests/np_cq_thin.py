"""
Host restatement of the thinned level-0 factor of the cq pair route (mfgm_cq_factor_pair_thin / mfgm_cq_selinv_kl_thin,
csrc/mfgm_cq.h), in fp64 and np.longdouble.

The forward sweep leaves per node the P-form record  P_t = F_t^{-1},  z_t = P_t h_t  with
    F_t = J_t - S_{t-1} P_{t-1} S_{t-1}^T,    h_t = r_t - S_{t-1} z_{t-1}        (J = -2 theta_diag, S = -theta_sub, r = theta_lin),
so record t follows from record t - 1, the transition into t and node t's own naturals.  The thinned route stores the records of
the KEPT nodes only -- local step s of a level-0 segment of length R is kept iff s is even or s == R - 1 -- and the backward sweep
rebuilds each of the others from the kept record before it with one step of that recursion.
"""
import numpy as np

from tests import np_cq

LD = np_cq.LD


def _T(x):
    return np.swapaxes(x, -1, -2)


# ---- the store rule -----------------------------------------------------------------------------------------------------------------------
def kept(s, R):
    """Whether the record at local step s of a segment of nominal length R is stored."""
    return s % 2 == 0 or s == R - 1


def kept_nodes(T, R):
    """Mask [T] over the nodes of a chain cut into segments of R nodes (the last one may be shorter)."""
    s = np.arange(T) % R
    return (s % 2 == 0) | (s == R - 1)


def stored_fraction(T, R):
    return float(kept_nodes(T, R).mean())


# ---- the recursion ------------------------------------------------------------------------------------------------------------------------
def _naturals(state, dtype):
    lin, diag, sub = (np.asarray(a, dtype=dtype) for a in np_cq.dense_naturals(state))
    return lin, -2 * diag, -sub


def forward_step(Pp, zp, S, J, r):
    """Record t from record t - 1: Pp [B, d, d], zp [B, d], S = -theta_sub of the transition [B, d, d], J = -2 theta_diag and
    r = theta_lin of node t (sites included).  The calls of the kernels' step in their order: carry, F / h, Cholesky, forward
    substitution, triangular inverse, X^T X, z."""
    d = Pp.shape[-1]
    C = S @ Pp @ _T(S)
    c = (S @ zp[..., None])[..., 0]
    L = np_cq.chol(J - C)
    y = np_cq.solve_lower(L, (r - c)[..., None])
    X = np_cq.solve_lower(L, np.broadcast_to(np.eye(d, dtype=Pp.dtype), Pp.shape))
    return _T(X) @ X, (_T(X) @ y)[..., 0], L


def forward_records(state, dtype=LD):
    """The full forward recursion over whole chains: (P [B, T, d, d], z [B, T, d], logdet [B] = sum of log diag of the factors)."""
    lin, J, S = _naturals(state, dtype)
    B, T, d = state.B, state.T, state.d
    P, z = np.empty((B, T, d, d), dtype=dtype), np.empty((B, T, d), dtype=dtype)
    logdet = np.zeros(B, dtype=dtype)
    Pp, zp, Sp = np.zeros((B, d, d), dtype=dtype), np.zeros((B, d), dtype=dtype), np.zeros((B, d, d), dtype=dtype)
    for t in range(T):
        P[:, t], z[:, t], L = forward_step(Pp, zp, Sp, J[:, t], lin[:, t])
        logdet += np.sum(np.log(np.diagonal(L, axis1=-2, axis2=-1)), axis=-1)
        Pp, zp = P[:, t], z[:, t]
        if t < T - 1:
            Sp = S[:, t]
    return P, z, logdet


def rebuilt_records(state, R, stored, dtype=LD):
    """What the thinned route works with: the stored records (P, z) at the kept nodes, and at every other node one forward step from
    the kept record before it.  `stored` = (P, z) of the full recursion; entries of unkept nodes are never read (they are poisoned
    here to show it)."""
    lin, J, S = _naturals(state, dtype)
    keep = kept_nodes(state.T, R)
    P, z = (np.array(a, dtype=dtype) for a in stored)
    P[:, ~keep], z[:, ~keep] = np.nan, np.nan
    Pout, zout = P.copy(), z.copy()
    for t in np.flatnonzero(~keep):
        assert keep[t - 1] and t % R != 0                # the node before a rebuilt one is a kept node of the same segment
        Pout[:, t], zout[:, t], _ = forward_step(P[:, t - 1], z[:, t - 1], S[:, t - 1], J[:, t], lin[:, t])
    return Pout, zout


# ---- an independent view of a record: np_cq's own elimination of the chain cut after node t ------------------------------------------------
def truncated(state, b, t):
    """Chain b of the state cut after node t, as a one-chain state of t + 1 nodes (its sites at nodes <= t, p0_off, the offsets).
    The last node of that chain has the marginal covariance P_t and the marginal mean z_t of the forward recursion: nothing after
    node t has been seen yet.  np_cq.posterior derives both on its own (Cholesky form, forward AND backward pass)."""
    from types import SimpleNamespace
    st = SimpleNamespace(**vars(state))
    st.B, st.T = 1, t + 1
    st.dyn = state.dyn[b:b + 1, :t + 1]
    if state.obs_t is not None:
        n = state.obs_t.shape[1]
        m = state.obs_t[b] <= t
        st.obs_t = state.obs_t[b][m][None] if m.any() else None
        st.site_lin = state.site_lin[b * n:(b + 1) * n][m] if m.any() else None
        if not m.any():
            st.site_sym = None
    return st
