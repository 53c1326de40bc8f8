"""
NumPy helpers of the sparse-CVI hyper-parameter tests (tests/test_host_sparse_hyper.py, tests/test_gpu_sparse_hyper.py; DESIGN.md
section 21); not a test module.  Kernel trees as in tests/np_hyper.py.

  (i)   SparseChain.elbo        a DENSE restatement of SparseCVIGaussianProcess.classic_elbo at given sites: the prior covariance of
                                the stacked inducing states, the posterior from the dense precision, KL[q || p] from dense matrices,
                                the conditionals in covariance form.  fd_gradient differences it centrally in each leaf in
                                np.longdouble with h = 1e-6 |leaf|: the yardstick.
  (ii)  conditional_score       the reverse-mode formulas of csrc/mfgm_sparse_score.h per data point, term and slot, written with
                                explicit n x n cotangent matrices (the kernel never forms them), any dtype.
  (iii) SparseChain.gradient    the whole gradient: the chain part as tests.np_hyper.score_restatement on moments displaced by the
                                DENSE Fisher-vector product  d Sigma = 2 Sigma V Sigma, d mu = Sigma (v + 2 V mu), plus (ii).
Gaussian and Poisson likelihoods: their variational expectations are closed forms.
"""
import math

import numpy as np

from tests import np_hyper as H

APPROX_INF = 1e10


# -- dtype-generic dense algebra -----------------------------------------------------------------------------------------------------------
def chol(K):
    return np.linalg.cholesky(K) if K.dtype == np.float64 else H._cholesky(K)


def spd_inverse(K):
    if K.dtype == np.float64:
        return np.linalg.inv(K)
    Li = H._solve_lower(chol(K), np.eye(K.shape[0], dtype=K.dtype))
    return Li.T @ Li


def spd_solve(K, B):
    if K.dtype == np.float64:
        return np.linalg.solve(K, B)
    L = chol(K)
    return H._solve_upper(L.T, H._solve_lower(L, B))


def logdet(K):
    return 2.0 * np.log(np.diag(chol(K))).sum()


# -- the kernel as (A, Q, Pinf) of the whole state ---------------------------------------------------------------------------------------------
def term_dims(spec):
    return [int(np.prod([H.LEAF_DIM[f[0]] for f in term])) for term in H.terms_of(spec)]


def transition(spec, jitter, dt, dtype):
    """(A, Q + jitter I, Pinf) of the whole state at the gap dt: block diagonal over the terms, Q under the exact-Q rule."""
    d = H.state_dim(spec)
    A, Q, P = (np.zeros((d, d), dtype=dtype) for _ in range(3))
    o = 0
    for term, n in zip(H.terms_of(spec), term_dims(spec)):
        a, p, q, _, _ = H.term_blocks(term, dtype(dt), dtype)
        A[o:o + n, o:o + n], P[o:o + n, o:o + n], Q[o:o + n, o:o + n] = a, p, q
        o += n
    return A, Q + dtype(jitter) * np.eye(d, dtype=dtype), P


def emission(spec, dtype):
    h = np.zeros(H.state_dim(spec), dtype=dtype)
    o = 0
    for n in term_dims(spec):
        h[o] = 1.0
        o += n
    return h


def gaps(t, z):
    """(interval index, t - z-, z+ - t): interval m lies between inducing points m - 1 and m, the ends padded at -/+ 1e10; a point ON
    an inducing point belongs to the interval on its left (searchsorted, side left)."""
    idx = np.searchsorted(z, t, side="left")
    aug = np.concatenate([[-APPROX_INF], z, [APPROX_INF]])
    return idx, t - aug[idx], aug[idx + 1] - t


def conditional_stats(spec, jitter, gap_lo, gap_hi, dtype):
    """w [N, 2d] and c [N] of p(f(t_i) | s(z-), s(z+)) in covariance form, term by term; a term whose Q_mp is exactly zero has x = 0."""
    d, N = H.state_dim(spec), len(gap_lo)
    w, c = np.zeros((N, 2 * d), dtype=dtype), np.zeros(N, dtype=dtype)
    for i in range(N):
        o = 0
        for term, n in zip(H.terms_of(spec), term_dims(spec)):
            A1, _, Q1, _, _ = H.term_blocks(term, dtype(gap_lo[i]), dtype)
            A2, _, Q2, _, _ = H.term_blocks(term, dtype(gap_hi[i]), dtype)
            eye = np.eye(n, dtype=dtype)
            Q1, Q2 = Q1 + dtype(jitter) * eye, Q2 + dtype(jitter) * eye
            h = eye[0]
            Qmp = Q2 + A2 @ Q1 @ A2.T
            x = spd_solve(Qmp, A2 @ Q1 @ h) if Qmp.any() else np.zeros(n, dtype=dtype)
            y = h - A2.T @ x
            w[i, o:o + n], w[i, d + o:d + o + n] = A1.T @ y, x
            c[i] += h @ Q1 @ y
            o += n
    return w, c


def conditional_score(spec, jitter, gap_lo, gap_hi, idx, M, a, b, wbar, wdata, dtype=np.float64):
    """Per-point contributions [N, nterm, 3, 2] to the (rate, var) score of  sum_i a_i fmu_i + b_i fvar_i  at fixed pair moments:
    wbar [N, 2d] = a mu_pair + 2 b Sigma_pair w is the cotangent of w, b that of c; wdata [N, 2d] the projections themselves (for the
    prior padding b w^T dPinf w of the intervals 0 and M).  Reverse mode through
        Q_mp = Q2 + A2 Q1 A2^T,  x = Q_mp^-1 A2 Q1 h,  y = h - A2^T x,  w+ = x,  w- = A1^T y,  c = h^T Q1 y
    with explicit cotangent matrices, pulled back through  Q = P - A P A^T + jitter I  and met by the factors' derivative blocks."""
    terms, dims = H.terms_of(spec), term_dims(spec)
    d, N = H.state_dim(spec), len(gap_lo)
    out = np.zeros((N, len(terms), 3, 2), dtype=dtype)
    for i in range(N):
        o = 0
        for c_, (term, n) in enumerate(zip(terms, dims)):
            d1, d2 = dtype(gap_lo[i]), dtype(gap_hi[i])
            A1, P, Q1, a1, p = H.term_blocks(term, d1, dtype)
            A2, _, Q2, a2, _ = H.term_blocks(term, d2, dtype)
            eye = np.eye(n, dtype=dtype)
            Q1, Q2 = Q1 + dtype(jitter) * eye, Q2 + dtype(jitter) * eye
            h = eye[0]
            wm, wp, cb = np.asarray(wbar[i, o:o + n], dtype=dtype), np.asarray(wbar[i, d + o:d + o + n], dtype=dtype), dtype(b[i])
            Qmp = Q2 + A2 @ Q1 @ A2.T
            zero = not Qmp.any()
            u = Q1 @ h
            x = np.zeros(n, dtype=dtype) if zero else spd_solve(Qmp, A2 @ u)
            y = h - A2.T @ x
            # reverse
            ub = cb * y                                   # c = u . y
            yb = cb * u + A1 @ wm                         # w- = A1^T y
            A1b = np.outer(y, wm)
            A2b = -np.outer(x, yb)                        # y = h - A2^T x
            xb = wp - A2 @ yb
            z = np.zeros(n, dtype=dtype) if zero else spd_solve(Qmp, xb)
            Qmpb = -np.outer(z, x)                        # x = Q_mp^-1 r
            Q2b = Qmpb
            Q1b = A2.T @ Qmpb @ A2
            A2b = A2b + (Qmpb + Qmpb.T) @ A2 @ Q1 + np.outer(z, u)      # Q_mp = Q2 + A2 Q1 A2^T;  r = A2 u
            ub = ub + A2.T @ z
            Q1b = Q1b + np.outer(ub, h)                   # u = Q1 h
            # Q = P - A P A^T + jitter I
            Pb = np.zeros((n, n), dtype=dtype)
            for Ab, Qb, A in ((A1b, Q1b, A1), (A2b, Q2b, A2)):
                Pb += Qb - A.T @ Qb @ A
                Ab -= (Qb + Qb.T) @ A @ P
            m = idx[i]
            if m == 0:
                wl = np.asarray(wdata[i, o:o + n], dtype=dtype)
                Pb += cb * np.outer(wl, wl)
            if m == M:
                wh = np.asarray(wdata[i, d + o:d + o + n], dtype=dtype)
                Pb += cb * np.outer(wh, wh)
            for f, leaf in enumerate(term):
                r, v = H.rate_var(leaf)
                rep = lambda blocks, new: H.kron_all([new if k == f else blocks[k] for k in range(len(term))])
                da1, dpl, dpv = H.factor_der(leaf[0], dtype(r), dtype(v), d1, dtype)
                da2, _, _ = H.factor_der(leaf[0], dtype(r), dtype(v), d2, dtype)
                out[i, c_, f, 0] = (A1b * rep(a1, da1)).sum() + (A2b * rep(a2, da2)).sum() + (Pb * rep(p, dpl)).sum()
                out[i, c_, f, 1] = (Pb * rep(p, dpv)).sum()
            o += n
    return out


# -- likelihoods -----------------------------------------------------------------------------------------------------------------------------
def ve_and_grads(lik, fmu, fvar, y):
    """(ve [N], d ve / d fmu, d ve / d fvar) of ("gaussian", variance) or ("poisson", binsize)."""
    kind, prm = lik
    dtype = fmu.dtype.type
    if kind == "gaussian":
        v = dtype(prm)
        ve = -0.5 * np.log(2 * dtype(np.pi) * v) - 0.5 * ((y - fmu) ** 2 + fvar) / v
        return ve, (y - fmu) / v, -0.5 / v * np.ones_like(fmu)
    bsz = dtype(prm)
    e = bsz * np.exp(fmu + 0.5 * fvar)
    lg = np.array([math.lgamma(float(v) + 1.0) for v in y], dtype=fmu.dtype)
    return y * np.log(bsz) + y * fmu - e - lg, y - e, -0.5 * e


# -- the model ---------------------------------------------------------------------------------------------------------------------------------
class SparseChain:
    """The sparse CVI model on M inducing points z and N sorted data points t, one kernel tree, dense."""

    def __init__(self, spec, jitter, z, t, y, lik, dtype=np.float64):
        self.spec, self.jitter, self.lik, self.dtype = spec, jitter, lik, dtype
        self.z, self.t, self.y = np.asarray(z, dtype=np.float64), np.asarray(t, dtype=np.float64), np.asarray(y, dtype=dtype)
        self.M, self.N, self.d = len(z), len(t), H.state_dim(spec)
        self.idx, self.gap_lo, self.gap_hi = gaps(self.t, self.z)
        M, d = self.M, self.d
        # the prior covariance of the stacked inducing states
        S = [transition(spec, jitter, 0.0, dtype)[2] + dtype(jitter) * np.eye(d, dtype=dtype)]
        As = []
        for k in range(M - 1):
            A, Q, _ = transition(spec, jitter, self.z[k + 1] - self.z[k], dtype)
            As.append(A)
            S.append(A @ S[-1] @ A.T + Q)
        K = np.zeros((M * d, M * d), dtype=dtype)
        for j in range(M):
            C = S[j]
            K[j * d:(j + 1) * d, j * d:(j + 1) * d] = C
            for i in range(j + 1, M):
                C = As[i - 1] @ C
                K[i * d:(i + 1) * d, j * d:(j + 1) * d] = C
                K[j * d:(j + 1) * d, i * d:(i + 1) * d] = C.T
        self.K = K
        self.P0 = S[0]
        self.Lam_p = spd_inverse(K)
        self.w, self.c = conditional_stats(spec, jitter, self.gap_lo, self.gap_hi, dtype)

    def zero_sites(self):
        return np.zeros((self.M + 1, 2 * self.d), dtype=self.dtype), np.zeros((self.M + 1, 2 * self.d, 2 * self.d), dtype=self.dtype)

    def dense_naturals(self, n1, n2):
        """(v [M d], V [M d, M d] symmetric) with  <theta, T(s)> = v . s + s^T V s  of pair sites: site k acts on the states (k - 1, k);
        what falls on the padding states at the two ends is dropped (mfgm_sparse_theta)."""
        M, d = self.M, self.d
        v, V = np.zeros(M * d, dtype=self.dtype), np.zeros((M * d, M * d), dtype=self.dtype)
        for k in range(M + 1):
            lo, hi = k - 1, k
            s2 = 0.5 * (n2[k] + n2[k].T)
            if lo >= 0:
                v[lo * d:(lo + 1) * d] += n1[k, :d]
                V[lo * d:(lo + 1) * d, lo * d:(lo + 1) * d] += s2[:d, :d]
            if hi < M:
                v[hi * d:(hi + 1) * d] += n1[k, d:]
                V[hi * d:(hi + 1) * d, hi * d:(hi + 1) * d] += s2[d:, d:]
            if lo >= 0 and hi < M:
                V[hi * d:(hi + 1) * d, lo * d:(lo + 1) * d] += s2[d:, :d]
                V[lo * d:(lo + 1) * d, hi * d:(hi + 1) * d] += s2[:d, d:]
        return v, V

    def posterior(self, n1, n2):
        """(mu [M d], Sigma [M d, M d]) of q = p exp<theta_s, T(s)> / Z."""
        v, V = self.dense_naturals(np.asarray(n1, dtype=self.dtype), np.asarray(n2, dtype=self.dtype))
        Sigma = spd_inverse(self.Lam_p - 2.0 * V)
        Sigma = 0.5 * (Sigma + Sigma.T)
        return Sigma @ v, Sigma

    def pair_moments(self, mu, Sigma):
        """mu_pair [M + 1, 2d], Sigma_pair [M + 1, 2d, 2d] per interval, the prior padding both ends."""
        M, d = self.M, self.d
        mp, Sp = np.zeros((M + 1, 2 * d), dtype=self.dtype), np.zeros((M + 1, 2 * d, 2 * d), dtype=self.dtype)
        blk = lambda i, j: Sigma[i * d:(i + 1) * d, j * d:(j + 1) * d]
        for k in range(M + 1):
            lo, hi = k - 1, k
            Sp[k, :d, :d] = blk(lo, lo) if lo >= 0 else self.P0
            Sp[k, d:, d:] = blk(hi, hi) if hi < M else self.P0
            if lo >= 0:
                mp[k, :d] = mu[lo * d:(lo + 1) * d]
            if hi < M:
                mp[k, d:] = mu[hi * d:(hi + 1) * d]
            if lo >= 0 and hi < M:
                Sp[k, d:, :d] = blk(hi, lo)
                Sp[k, :d, d:] = blk(lo, hi)
        return mp, Sp

    def predict(self, mu, Sigma):
        mp, Sp = self.pair_moments(mu, Sigma)
        fmu = np.einsum("ij,ij->i", self.w, mp[self.idx])
        fvar = self.c + np.einsum("ij,ijk,ik->i", self.w, Sp[self.idx], self.w)
        return fmu, fvar, mp, Sp

    def elbo(self, n1, n2):
        mu, Sigma = self.posterior(n1, n2)
        fmu, fvar, _, _ = self.predict(mu, Sigma)
        ve = ve_and_grads(self.lik, fmu, fvar, self.y)[0].sum()
        n = self.M * self.d
        kl = 0.5 * ((self.Lam_p * Sigma).sum() + mu @ self.Lam_p @ mu - n + logdet(self.K) - logdet(Sigma))
        return ve - kl

    def cvi_target(self, n1, n2):
        """(g^1 [M + 1, 2d], g^2 [M + 1, 2d, 2d], a, b, fmu, fvar, pair moments): the sites a CVI step at lr = 1 would write."""
        mu, Sigma = self.posterior(n1, n2)
        fmu, fvar, mp, Sp = self.predict(mu, Sigma)
        _, a, b = ve_and_grads(self.lik, fmu, fvar, self.y)
        g1, g2 = a - 2.0 * b * fmu, b
        t1, t2 = self.zero_sites()
        for i in range(self.N):
            t1[self.idx[i]] += g1[i] * self.w[i]
            t2[self.idx[i]] += g2[i] * np.outer(self.w[i], self.w[i])
        return t1, t2, a, b, (mu, Sigma, mp, Sp)

    def update_sites(self, n1, n2, lr):
        t1, t2 = self.cvi_target(n1, n2)[:2]
        return (1 - lr) * n1 + lr * t1, (1 - lr) * n2 + lr * t2

    def gradient(self, n1, n2, parts=None):
        """Flat leaf gradients of elbo at fixed sites (the order of np_hyper.flat_params).  parts (a dict) receives the three
        contributions: chain_kl, chain_fisher, conditional."""
        M, d, dtype = self.M, self.d, self.dtype
        n1, n2 = np.asarray(n1, dtype=dtype), np.asarray(n2, dtype=dtype)
        t1, t2, a, b, (mu, Sigma, mp, Sp) = self.cvi_target(n1, n2)
        # F (g^ - theta_s) from the dense posterior covariance
        v, V = self.dense_naturals(t1 - n1, t2 - n2)
        dSigma = 2.0 * Sigma @ V @ Sigma
        dmu = Sigma @ (v + 2.0 * V @ mu)
        dS = dSigma + np.outer(dmu, mu) + np.outer(mu, dmu)
        blk = lambda X, i, j: X[i * d:(i + 1) * d, j * d:(j + 1) * d]
        x = mu.reshape(M, d)
        Sig = np.stack([blk(Sigma, k, k) for k in range(M)])
        Sub = np.stack([blk(Sigma, k + 1, k) for k in range(M - 1)])
        dSig = np.stack([blk(dS, k, k) for k in range(M)])
        dSub = np.stack([blk(dS, k + 1, k) for k in range(M - 1)])
        dz = np.diff(self.z)
        kl = H.leaves_from_score(self.spec, H.score_restatement(self.spec, self.jitter, dz, x, Sig, Sub, dtype=dtype))
        both = H.leaves_from_score(self.spec, H.score_restatement(self.spec, self.jitter, dz, x, Sig + dSig, Sub + dSub, dtype=dtype))
        wbar = a[:, None] * mp[self.idx] + 2.0 * b[:, None] * np.einsum("ijk,ik->ij", Sp[self.idx], self.w)
        per_point = conditional_score(self.spec, self.jitter, self.gap_lo, self.gap_hi, self.idx, M, a, b, wbar, self.w, dtype=dtype)
        cond = H.leaves_from_score(self.spec, per_point.sum(0))
        if parts is not None:
            parts.update(chain_kl=kl, chain_fisher=both - kl, conditional=cond)
        return both + cond


def fd_gradient(spec, jitter, z, t, y, lik, n1, n2, rel_step=1e-6):
    """Central differences of the dense np.longdouble ELBO at fixed sites in each leaf, h = rel_step |leaf|: the yardstick."""
    ld = np.longdouble
    params = [ld(p) for p in H.flat_params(spec)]
    n1, n2 = np.asarray(n1, dtype=ld), np.asarray(n2, dtype=ld)
    out = []
    for k, p in enumerate(params):
        h = ld(rel_step) * abs(p)
        vals = []
        for s in (+1, -1):
            q = list(params)
            q[k] = p + s * h
            vals.append(SparseChain(H.with_params(spec, q), jitter, z, t, y, lik, dtype=ld).elbo(n1, n2))
        out.append((vals[0] - vals[1]) / (2 * h))
    return np.array(out, dtype=ld)


def make_problem(rng, spec, M, N, lik_kind, min_gap=0.5):
    """(z [M], t [N] sorted, y [N]): inducing points with gaps >= min_gap of the tree's shortest time scale, data points uniform over
    a range that reaches into both end intervals, each at least that far from every inducing point."""
    lm = H.shortest_lengthscale(spec)
    lm = 1.0 if not np.isfinite(lm) else lm
    z = np.cumsum(rng.uniform(2.0 * min_gap, 3.0 * min_gap, M) * lm * 2.0)
    cells = np.concatenate([[z[0] - 3.0 * min_gap * lm], z, [z[-1] + 3.0 * min_gap * lm]])
    k = rng.integers(0, M + 1, N)
    k[:2] = (0, M)
    lo, hi = cells[k] + min_gap * lm, cells[k + 1] - min_gap * lm
    t = np.sort(lo + rng.uniform(0, 1, N) * (hi - lo))
    f = 0.8 * np.sin(t / (2.0 * lm)) + 0.3 * rng.normal(size=N)
    y = rng.poisson(np.exp(f)).astype(np.float64) if lik_kind == "poisson" else f + 0.3 * rng.normal(size=N)
    return z, t, y
