"""
Host restatement of the level-0 reduce with the observed nodes eliminated last (mfgm_cq_factor_pair_heads, csrc/mfgm_cq.h), in fp64
and np.longdouble, next to the plain sequential reduce, and the generator of the cq states the host and GPU tests of that entry share.

A level-0 reduce gives, per segment p of a chain (nodes t0 ... t0 + len - 1, separator = the last one), five blocks:
    Dhat, rhat   the separator's diagonal block and right-hand side with the segment's interior eliminated,
    S            the spike that couples separator p - 1 to separator p,
    Rsub, rho    what separator p - 1 loses to the interior (its block is Dhat[p - 1] - Rsub[p], its right-hand side rhat[p - 1] - rho[p]).
They are the Schur complement of the interiors onto the separators, which no elimination order changes.  `separator_posterior` solves
that separator system, so that either reduce can be held to the whole-chain elimination of tests/np_cq.py.
"""
from types import SimpleNamespace

import numpy as np

from tests import np_cq

LD = np_cq.LD
# (B, T, R0, Rup, q): observations on multiples of q, R0 a multiple of q
#   m = 2, a one-node last segment that is an observed head | m = 3, a ragged last segment with a one-node last interior |
#   four tiles with padding lanes, empty interiors, chains of three segments | m = 1 | an exact multiple with every head observed
SHAPES = [(3, 257, 8, 3, 4), (3, 259, 12, 3, 4), (70, 9, 4, 3, 2), (1, 33, 16, 3, 16), (2, 64, 16, 3, 8)]
SHAPE_IDS = ["B3-T257-R8-q4", "B3-T259-R12-q4", "B70-T9-R4-q2", "B1-T33-R16-q16", "B2-T64-R16-q8"]
DIMS = [1, 2, 3, 6, 8]


def _T(x):
    return np.swapaxes(x, -1, -2)


# ---- the generator ------------------------------------------------------------------------------------------------------------------------
def make_state(d, shape, seed=0):
    """np_cq.make_state(..., sites=False) plus observations on multiples of q: every chain has the same number of them on its own
    subset of the heads; the last head, T - 1 where it is a head, and node 0 are forced -- node 0 in every chain but the last one of
    a batch (so B > 1 has a chain whose node 0 is not observed) unless every head is observed (the last shape)."""
    B, T, R0, Rup, q = shape
    st = np_cq.make_state(d, (B, T, R0, Rup), seed=seed, sites=False)
    assert st.levels[0][1] % q == 0, "the level-0 segment length must be a multiple of the observation spacing"
    rng = np.random.default_rng([71892305, d, B, T, q, seed])
    heads = np.arange(0, T, q)
    every = shape == SHAPES[-1]
    n = len(heads) if every else max(2, (len(heads) + 2) // 2)
    rows = []
    for b in range(B):
        forced = {int(heads[-1])}
        if every or B == 1 or b < B - 1:
            forced.add(0)
        free = np.array([t for t in heads if t not in forced and (t != 0 or every)])
        pick = rng.choice(free, size=n - len(forced), replace=False) if n > len(forced) else np.array([], dtype=int)
        rows.append(rng.permutation(np.concatenate([np.array(sorted(forced)), pick]).astype(np.int64)))
    st.obs_t = np.stack(rows)
    A = rng.normal(size=(d, d))
    st.site_sym = -0.5 * (A @ A.T / d + 0.5 * np.eye(d))
    st.site_lin = rng.normal(size=(B * n, d))
    st.y = rng.normal(size=(B, n, d))
    st.cholR = 0.3 * np.eye(d) + 0.1 * np.eye(d, k=-1)
    st.q = q
    return st


def without_sites(st):
    s = SimpleNamespace(**vars(st))
    s.obs_t = s.site_lin = s.site_sym = None
    return s


# ---- d <= 8 linear algebra that keeps the dtype it is given ---------------------------------------------------------------------------------
def _chol(A):
    d = A.shape[-1]
    L = np.zeros_like(A)
    for j in range(d):
        s = A[..., j, j] - np.sum(L[..., j, :j] * L[..., j, :j], axis=-1)
        assert np.all(s > 0), "block is not positive definite"
        L[..., j, j] = np.sqrt(s)
        for i in range(j + 1, d):
            L[..., i, j] = (A[..., i, j] - np.sum(L[..., i, :j] * L[..., j, :j], axis=-1)) / L[..., j, j]
    return L


def _solve_lower(L, M):
    X = np.array(M)
    for i in range(L.shape[-1]):
        X[..., i, :] = (X[..., i, :] - np.sum(L[..., i, :i, None] * X[..., :i, :], axis=-2)) / L[..., i, i, None]
    return X


def _blocks(state, dtype):
    """Scaled blocks of the precision: A [B, T, d, d] = -2 theta_diag, Bs [B, T - 1, d, d] = -theta_sub (couples t -> t + 1),
    r [B, T, d, 1]."""
    lin, diag, sub = np_cq.dense_naturals(state)
    return (-2 * diag).astype(dtype), (-sub).astype(dtype), lin[..., None].astype(dtype)


def _step(F, W, h, Racc, rho, Bn):
    """One elimination step: returns (G G^T, -G W', G y) -- what the next node's block loses, the spike from the next node, what its
    right-hand side loses -- and the updated accumulators."""
    L = _chol(F)
    W = _solve_lower(L, W)
    Racc = Racc + _T(W) @ W
    y = _solve_lower(L, h)
    rho = rho + _T(W) @ y
    G = _T(_solve_lower(L, _T(Bn)))
    return G @ _T(G), -G @ W, G @ y, Racc, rho


def _segments(state):
    n, R, P, _ = state.levels[0]
    return [(p, p * R, min(R, n - p * R)) for p in range(P)]


def _empty(state, dtype):
    B, d, P = state.B, state.d, state.levels[0][2]
    z = lambda *s: np.zeros((B, P) + s, dtype=dtype)
    return dict(Dhat=z(d, d), rhat=z(d, 1), S=z(d, d), Rsub=z(d, d), rho=z(d, 1))


def reduce_sequential(state, dtype=LD):
    """The reduce as reduce_cq_body makes it: nodes eliminated left to right."""
    A, Bs, r = _blocks(state, dtype)
    out = _empty(state, dtype)
    B, d = state.B, state.d
    for p, t0, ln in _segments(state):
        F, h = A[:, t0], r[:, t0]
        W = Bs[:, t0 - 1] if p > 0 else np.zeros((B, d, d), dtype=dtype)
        Racc, rho = np.zeros((B, d, d), dtype=dtype), np.zeros((B, d, 1), dtype=dtype)
        for s in range(ln - 1):
            GG, W, Gy, Racc, rho = _step(F, W, h, Racc, rho, Bs[:, t0 + s])
            F, h = A[:, t0 + s + 1] - GG, r[:, t0 + s + 1] - Gy
        for name, v in zip(("Dhat", "rhat", "S", "Rsub", "rho"), (F, h, W, Racc, rho)):
            out[name][:, p] = v
    return out


def reduce_heads_last(state, q, dtype=LD):
    """The same five blocks with the heads (local steps 0, q, 2q, ... below len) and the segment's last node kept to the end.
    Shared part: per pair of consecutive kept nodes (lo, hi) the recurrence over lo + 1 ... hi - 1 with lo in the role of the left
    separator, on the blocks WITHOUT any site or p0_off; parked (F', h', V, Racc, rho).  Tail: one step per sub-segment with V in the
    place of theta_sub; a kept node takes its parked block, its own site term and what its own interior took."""
    A, Bs, r = _blocks(state, dtype)                       # with sites and p0_off: what the kept nodes carry
    A0, _, r0 = _blocks(SimpleNamespace(**{**vars(without_sites(state)), "p0_off": None}), dtype)
    assert state.levels[0][1] % q == 0
    out = _empty(state, dtype)
    B, d = state.B, state.d
    zero = lambda *s: np.zeros((B,) + s, dtype=dtype)
    for p, t0, ln in _segments(state):
        kept = sorted(set(range(0, ln, q)) | {ln - 1})
        # every node that carries a site or p0_off is a head
        for s in range(ln):
            if s % q:
                assert np.array_equal(A[:, t0 + s], A0[:, t0 + s]) and np.array_equal(r[:, t0 + s], r0[:, t0 + s])
        parked = []
        for lo, hi in zip(kept[:-1], kept[1:]):
            F, h, W = A0[:, t0 + lo + 1], r0[:, t0 + lo + 1], Bs[:, t0 + lo]
            Racc, rho = zero(d, d), zero(d, 1)
            for s in range(lo + 1, hi):
                GG, W, Gy, Racc, rho = _step(F, W, h, Racc, rho, Bs[:, t0 + s])
                F, h = A0[:, t0 + s + 1] - GG, r0[:, t0 + s + 1] - Gy
            parked.append((F, h, W, Racc, rho))
        site_A = lambda s: A[:, t0 + s] - A0[:, t0 + s]
        site_r = lambda s: r[:, t0 + s] - r0[:, t0 + s]
        F, h = A[:, t0], r[:, t0]
        if parked:
            F, h = F - parked[0][3], h - parked[0][4]
        W = Bs[:, t0 - 1] if p > 0 else zero(d, d)
        Racc, rho = zero(d, d), zero(d, 1)
        for k, (Fp, hp, V, _, _) in enumerate(parked):
            GG, W, Gy, Racc, rho = _step(F, W, h, Racc, rho, V)
            hi = kept[k + 1]
            F, h = Fp - GG, hp - Gy
            if hi % q == 0:
                F, h = F + site_A(hi), h + site_r(hi)
            if k + 1 < len(parked):
                F, h = F - parked[k + 1][3], h - parked[k + 1][4]
        for name, v in zip(("Dhat", "rhat", "S", "Rsub", "rho"), (F, h, W, Racc, rho)):
            out[name][:, p] = v
    return out


def separator_posterior(state, red):
    """Mean and covariance of the separator nodes from a reduce's five blocks (longdouble): sequential block elimination along the
    separator chain with the routines of tests/np_cq.py, then the backward recursion of np_cq.posterior.  Returns (nodes [P], x
    [B, P, d], Sig [B, P, d, d])."""
    B, d = state.B, state.d
    segs = _segments(state)
    P = len(segs)
    red = {k: np.asarray(v, dtype=LD) for k, v in red.items()}
    J = red["Dhat"].copy()
    rhs = red["rhat"].copy()
    J[:, :P - 1] -= red["Rsub"][:, 1:]
    rhs[:, :P - 1] -= red["rho"][:, 1:]
    Sc = red["S"][:, 1:]                                   # [B, P - 1]: couples separator p -> p + 1
    eye = np.broadcast_to(np.eye(d, dtype=LD), (B, d, d))
    Ls, Gs, ys = [], [], []
    carry, cy = np.zeros((B, d, d), dtype=LD), np.zeros((B, d, 1), dtype=LD)
    for p in range(P):
        L = np_cq.chol(J[:, p] - carry)
        y = np_cq.solve_lower(L, rhs[:, p] - cy)
        Ls.append(L)
        ys.append(y)
        if p < P - 1:
            G = _T(np_cq.solve_lower(L, _T(Sc[:, p])))
            Gs.append(G)
            carry, cy = G @ _T(G), G @ y
    x = np.empty((B, P, d), dtype=LD)
    Sig = np.empty((B, P, d, d), dtype=LD)
    for p in range(P - 1, -1, -1):
        Li = np_cq.solve_lower(Ls[p], eye)
        base, rh = _T(Li) @ Li, ys[p]
        if p < P - 1:
            H = Gs[p] @ Li
            base = base + _T(H) @ Sig[:, p + 1] @ H
            rh = rh - _T(Gs[p]) @ x[:, p + 1, :, None]
        Sig[:, p] = (base + _T(base)) / 2
        x[:, p] = np_cq.solve_lower_t(Ls[p], rh)[..., 0]
    nodes = np.array([t0 + ln - 1 for _, t0, ln in segs])
    return nodes, x, Sig
