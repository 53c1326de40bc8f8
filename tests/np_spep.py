"""
Dense NumPy model of sparse Power Expectation Propagation (vidp_amd.sparse_pep; include/mfgm.h, mfgm_sparse_pep_sites), written from
the algorithm of DESIGN.md section 14 with no state-space structure: the joint prior precision over all inducing states as one dense
matrix, the sites as dense [2d, 2d] blocks overlap-added into it, the posterior by one dense inverse, the cavities by dense
[2d, 2d] inverses (route "inverse") or Cholesky solves (route "cholesky").

Intervals m = 0..M lie between inducing states m - 1 and m; the prior's initial state pads both ends (independent of the chain), so the
pair marginal of interval 0 is blockdiag(P0, S_00) and the padded half of the end sites does not enter the posterior.
"""
import numpy as np

from oracle import np_conditionals
from tests import np_pep

LOG2PI = np_pep.LOG2PI


def data_terms(kernel, z, t):
    """(seg [M + 2], w [N, 2d], c [N]) of sorted time points t: CSR offsets per interval, w_i = H P_i, c_i = H T_i H^T."""
    P, T, idx = np_conditionals.conditional_statistics(np.asarray(t, dtype=np.float64), np.asarray(z, dtype=np.float64), kernel)
    h = kernel.emission_vector()[0]
    seg = np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=len(z) + 1))]).astype(np.int64)
    return seg, np.einsum("i,nij->nj", h, P), np.einsum("i,nij,j->n", h, T, h)


def _spd(A):
    return np.linalg.eigvalsh(0.5 * (A + np.swapaxes(A, -1, -2))).min(-1) > 0


def interval_update(kind, seg, w, c, y, mu, S, nat1, nat2, lnorm, param, alpha, lr, route="inverse", scales=False):
    """One sparse PEP update of every interval from given pair marginals (mu [M+1, n], S [M+1, n, n]): returns (nat1, nat2, lnorm, e
    [M+1], skipped) and, with scales=True, the sums of absolute terms (s1, s2, s3, se) of the four outputs."""
    M1, n = mu.shape
    seg = np.asarray(seg)
    cnt = np.diff(seg)
    has = cnt > 0
    idx = np.repeat(np.arange(M1), cnt)
    beta = alpha / np.maximum(cnt, 1)
    eye = np.eye(n)
    with np.errstate(all="ignore"):
        ok = _spd(S)
        Ss = np.where(ok[:, None, None], S, eye)
        if route == "inverse":
            Lam = np.linalg.inv(Ss)
            ldS = np.linalg.slogdet(Ss)[1]
        else:
            L = np.linalg.cholesky(Ss)
            Li = np.linalg.solve(L, np.broadcast_to(eye, Ss.shape))
            Lam = np.swapaxes(Li, -1, -2) @ Li
            ldS = 2.0 * np.log(np.diagonal(L, axis1=-2, axis2=-1)).sum(-1)
        h = (Lam @ mu[..., None])[..., 0]
        gq = 0.5 * (ldS + (mu * h).sum(-1))
        Lc = Lam + 2.0 * beta[:, None, None] * nat2
        hc = h - beta[:, None] * nat1
        okc = _spd(Lc)
        ok &= okc
        Lcs = np.where(okc[:, None, None], Lc, eye)
        if route == "inverse":
            Sc = np.linalg.inv(Lcs)
            ldC = np.linalg.slogdet(Lcs)[1]
        else:
            L = np.linalg.cholesky(Lcs)
            Li = np.linalg.solve(L, np.broadcast_to(eye, Lcs.shape))
            Sc = np.swapaxes(Li, -1, -2) @ Li
            ldC = 2.0 * np.log(np.diagonal(L, axis1=-2, axis2=-1)).sum(-1)
        muc = (Sc @ hc[..., None])[..., 0]
        gc = 0.5 * (-ldC + (hc * muc).sum(-1))
        ok |= ~has
        N = len(idx)
        s, mc, smc = np.zeros(N), np.zeros(N), np.zeros(N)
        for k in range(int(cnt.max()) if N else 0):          # the k-th point of every interval that has one: no [N, n, n] gather
            sel = np.nonzero(cnt > k)[0]
            i = seg[sel] + k
            s[i] = np.einsum("pi,pij,pj->p", w[i], Sc[sel], w[i])
            mc[i] = (w[i] * muc[sel]).sum(-1)
            smc[i] = (np.abs(w[i]) * np.abs(muc[sel])).sum(-1)
        lz, d1, d2, sc = np_pep.tilted(kind, mc, s + c, y, param, alpha)
        L2 = 0.5 / (s + 1.0 / d2)
        L1 = 2.0 * L2 * (d1 / d2 - mc)
        fin = np.isfinite(L1) & np.isfinite(L2)
        L1z, L2z = np.where(fin, L1, 0.0), np.where(fin, L2, 0.0)
        e = np.bincount(idx, weights=np.where(fin, lz + (gc - gq)[idx], 0.0), minlength=M1)
        d1s, d2s = np.zeros_like(nat1), np.zeros_like(nat2)
        np.add.at(d1s, idx, L1z[:, None] * w)
        for k in range(int(cnt.max()) if N else 0):
            sel = np.nonzero(cnt > k)[0]
            i = seg[sel] + k
            d2s[sel] += L2z[i, None, None] * w[i][:, :, None] * w[i][:, None, :]
        new = [(1 - lr) * X + lr * ((1 - alpha) * X + dX) for X, dX in ((nat1, d1s), (nat2, d2s), (lnorm, e))]
        out1 = np.where(ok[:, None], new[0], nat1)
        out2 = np.where(ok[:, None, None], new[1], nat2)
        out3 = np.where(ok, new[2], lnorm)
        e = np.where(ok, e, np.nan)
        skipped = int(cnt[~ok].sum() + (~fin & ok[idx]).sum())
        if not scales:
            return out1, out2, out3, e, skipped
        # sums of absolute terms, with the conditioning of L2 = 1/2 / (s + 1/d2) and of d1/d2 - mc carried through (tests/test_gpu_pep.py)
        k2 = (s + 1.0 / np.abs(d2)) / np.abs(s + 1.0 / d2) * (1.0 + sc["d2"] / np.abs(d2))
        r = d1 / d2
        k1 = (np.abs(r) * (1.0 + sc["d1"] / np.maximum(np.abs(d1), 1e-300) + sc["d2"] / np.abs(d2)) + smc) / np.abs(r - mc)
        sL1, sL2 = np.abs(L1) * (1.0 + k2 + k1), np.abs(L2) * (1.0 + k2)
        a1s, a2s = np.zeros_like(nat1), np.zeros_like(nat2)
        np.add.at(a1s, idx, sL1[:, None] * np.abs(w))
        for k in range(int(cnt.max()) if N else 0):
            sel = np.nonzero(cnt > k)[0]
            i = seg[sel] + k
            a2s[sel] += sL2[i, None, None] * np.abs(w[i])[:, :, None] * np.abs(w[i])[:, None, :]
        ge = np.abs(ldC) + np.abs(ldS) + (np.abs(hc) * np.abs(muc)).sum(-1) + (np.abs(mu) * np.abs(h)).sum(-1)
        se = np.bincount(idx, weights=np.abs(lz) + 1.0 + 0.5 * ge[idx], minlength=M1) + 1e-300
        s1 = np.abs((1 - lr) * nat1) + lr * (np.abs((1 - alpha) * nat1) + a1s) + 1e-300
        s2 = np.abs((1 - lr) * nat2) + lr * (np.abs((1 - alpha) * nat2) + a2s) + 1e-300
        s3 = np.abs((1 - lr) * lnorm) + lr * (np.abs((1 - alpha) * lnorm) + se)
        return out1, out2, out3, e, skipped, (s1, s2, s3, se)


def gaussian_closed_form(K_uu, W, c, y, s2, alpha):
    """Fixed-point energy of a Gaussian likelihood when no interval holds more than one point:
    log N(y; 0, W K_uu W^T + diag(alpha c + s^2)) - (1 - alpha) / (2 alpha) sum_i log(1 + alpha c_i / s^2)."""
    C = W @ K_uu @ W.T + np.diag(alpha * c + s2)
    L = np.linalg.cholesky(C)
    r = np.linalg.solve(L, y)
    lml = -0.5 * len(y) * LOG2PI - np.log(np.diag(L)).sum() - 0.5 * r @ r
    return lml - (1.0 - alpha) / (2.0 * alpha) * np.log1p(alpha * c / s2).sum()


class SparsePowerExpectationPropagation:
    """The dense model: kernel from oracle/np_kernels (zero state mean), inducing points z [M], likelihood kind / param as np_pep."""

    def __init__(self, kernel, inducing_points, kind, param, learning_rate=1.0, alpha=1.0, ve=None):
        self.kernel, self.z = kernel, np.asarray(inducing_points, dtype=np.float64)
        self.kind, self.param, self.lr, self.alpha, self.ve = kind, float(param), learning_rate, alpha, ve
        self.M, self.d = len(self.z), kernel.state_dim
        n = 2 * self.d
        self.nat1 = np.zeros((self.M + 1, n))
        self.nat2 = np.tile(-1e-10 * np.eye(n), (self.M + 1, 1, 1))
        self.log_norm = np.zeros(self.M + 1)
        self.Pp = np_pep.dense_precision(kernel.state_space_model(self.z))
        self.P0 = kernel.initial_covariance()
        self.skipped = 0

    def site_embedding(self, nat1, nat2):
        """(b, -2 x the overlap-added nat2) over the chain's M d numbers: the padded halves of the end sites fall outside."""
        M, d = self.M, self.d
        b, Q = np.zeros((M + 2) * d), np.zeros(((M + 2) * d, (M + 2) * d))
        for m in range(M + 1):
            sl = slice(m * d, (m + 2) * d)
            b[sl] += nat1[m]
            Q[sl, sl] += -2.0 * nat2[m]
        return b[d:-d], Q[d:-d, d:-d]

    def posterior(self, nat1=None, nat2=None):
        b, Q = self.site_embedding(self.nat1 if nat1 is None else nat1, self.nat2 if nat2 is None else nat2)
        P = self.Pp + Q
        S = np.linalg.inv(P)
        return P, S @ b, S

    def pair_marginals(self, nat1=None, nat2=None):
        M, d = self.M, self.d
        _, mu, S = self.posterior(nat1, nat2)
        em = np.zeros((M + 2) * d)
        em[d:-d] = mu
        eS = np.zeros(((M + 2) * d, (M + 2) * d))
        eS[d:-d, d:-d] = S
        eS[:d, :d] = self.P0
        eS[-d:, -d:] = self.P0
        return (np.stack([em[m * d:(m + 2) * d] for m in range(M + 1)]),
                np.stack([eS[m * d:(m + 2) * d, m * d:(m + 2) * d] for m in range(M + 1)]))

    def _update(self, t, y, lr, route="inverse"):
        seg, w, c = data_terms(self.kernel, self.z, t)
        mu, S = self.pair_marginals()
        return interval_update(self.kind, seg, w, c, np.asarray(y, dtype=np.float64).reshape(-1), mu, S, self.nat1, self.nat2,
                               self.log_norm, self.param, self.alpha, lr, route)

    def update_sites(self, t, y):
        self.nat1, self.nat2, self.log_norm, _, sk = self._update(t, y, self.lr)
        self.skipped += sk

    def compute_log_norm(self, t, y):
        return self._update(t, y, 0.0)[3]

    def energy(self, t, y):
        P, mu, _ = self.posterior()
        return (np_pep.normalizer(P, mu) - np_pep.normalizer(self.Pp, np.zeros(len(mu)))
                + self.compute_log_norm(t, y).sum() / self.alpha)

    def predict_f(self, t):
        seg, w, c = data_terms(self.kernel, self.z, t)
        idx = np.repeat(np.arange(self.M + 1), np.diff(seg))
        mu, S = self.pair_marginals()
        return (w * mu[idx]).sum(-1), np.einsum("pi,pij,pj->p", w, S[idx], w) + c

    def classic_elbo(self, t, y):
        """sum_i E_q log p(y_i | f_i) - KL[q(u) || p(u)], dense; `ve(mu, var, y)` gives the variational expectations."""
        fmu, fvar = self.predict_f(t)
        _, mu, S = self.posterior()
        k = len(mu)
        kl = 0.5 * (np.trace(self.Pp @ S) + mu @ self.Pp @ mu - k - np.linalg.slogdet(self.Pp)[1] - np.linalg.slogdet(S)[1])
        return np.sum(self.ve(fmu, fvar, np.asarray(y, dtype=np.float64).reshape(-1))) - kl
