"""
NumPy helpers of the panel hyper-parameter tests (tests/test_host_panel_hyper.py, tests/test_gpu_panel_hyper.py; DESIGN.md section
27); not a test module.  The panel has no restatement of its own: it is B single chains that share a kernel, so

  (i)   Panel.elbo / Panel.gradient    the sums over the rows of tests.np_sparse_hyper.SparseChain.elbo / .gradient, every series built
                                       from its present points only (a NaN observation is simply not there), at the series' own sites;
  (ii)  fd_gradient                    the sum of np_sparse_hyper.fd_gradient (central differences of the dense np.longdouble ELBO)
                                       over the rows: the yardstick;
  (iii) conditional_score              np_sparse_hyper.conditional_score per point of every series on packed-free inputs: pair
                                       moments in natural layout [B, M, ...], the prior padding both ends.
Gaussian and Poisson as np_sparse_hyper; Bernoulli through the 20-node rule of tests/np_lik.py (float64 only).
"""
import numpy as np

from tests import np_hyper as H
from tests import np_lik
from tests import np_sparse_hyper as S


class Series(S.SparseChain):
    """SparseChain with the Bernoulli likelihood ("bernoulli", jitter) added: the two methods that evaluate the likelihood."""

    def _lik(self, fmu, fvar):
        if self.lik[0] != "bernoulli":
            return S.ve_and_grads(self.lik, fmu, fvar, self.y)
        return np_lik.Bernoulli(self.lik[1]).ve_and_grads(fmu, fvar, self.y)[:3]

    def elbo(self, n1, n2):
        mu, Sigma = self.posterior(n1, n2)
        fmu, fvar, _, _ = self.predict(mu, Sigma)
        n = self.M * self.d
        kl = 0.5 * ((self.Lam_p * Sigma).sum() + mu @ self.Lam_p @ mu - n + S.logdet(self.K) - S.logdet(Sigma))
        return self._lik(fmu, fvar)[0].sum() - kl

    def cvi_target(self, n1, n2):
        mu, Sigma = self.posterior(n1, n2)
        fmu, fvar, mp, Sp = self.predict(mu, Sigma)
        _, a, b = self._lik(fmu, fvar)
        g1, g2 = a - 2.0 * b * fmu, b
        t1, t2 = self.zero_sites()
        for i in range(self.N):
            t1[self.idx[i]] += g1[i] * self.w[i]
            t2[self.idx[i]] += g2[i] * np.outer(self.w[i], self.w[i])
        return t1, t2, a, b, (mu, Sigma, mp, Sp)


def present(t, y):
    """[(t_b[keep], y_b[keep]) per row] of t [B, N], y [B, N] with NaN for an absent point."""
    return [(tb[~np.isnan(yb)], yb[~np.isnan(yb)]) for tb, yb in zip(t, y)]


class Panel:
    """B series on one kernel tree and one inducing grid z; t, y [B, N], NaN observations absent."""

    def __init__(self, spec, jitter, z, t, y, lik, dtype=np.float64):
        self.series = [Series(spec, jitter, z, tb, yb, lik, dtype=dtype) for tb, yb in present(t, y)]

    def zero_sites(self):
        n1, n2 = zip(*[s.zero_sites() for s in self.series])
        return np.stack(n1), np.stack(n2)

    def update_sites(self, n1, n2, lr):
        out = [s.update_sites(a, b, lr) for s, a, b in zip(self.series, n1, n2)]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])

    def elbo(self, n1, n2):
        return sum(s.elbo(a, b) for s, a, b in zip(self.series, n1, n2))

    def gradient(self, n1, n2, parts=None):
        """Flat leaf gradients of elbo at fixed sites, summed over the series; parts (a dict) receives the three contributions."""
        total, acc = 0.0, {}
        for s, a, b in zip(self.series, n1, n2):
            p = {}
            total = total + s.gradient(a, b, p)
            for k, v in p.items():
                acc[k] = acc.get(k, 0.0) + v
        if parts is not None:
            parts.update(acc)
        return total


def panel_problem(rng, spec, B, M, N, lik_kind, absent=0.15):
    """(z [M], t [B, N] sorted rows, y [B, N] with about `absent` of the entries NaN): np_sparse_hyper.make_problem row by row on one
    inducing grid; every row keeps at least one point."""
    z, _, _ = S.make_problem(rng, spec, M, N, lik_kind)
    lm = H.shortest_lengthscale(spec)
    lm = 1.0 if not np.isfinite(lm) else lm
    cells = np.concatenate([[z[0] - 1.5 * lm], z, [z[-1] + 1.5 * lm]])
    t, y = np.zeros((B, N)), np.zeros((B, N))
    for b in range(B):
        k = rng.integers(0, M + 1, N)
        k[:2] = (0, M)
        lo, hi = cells[k] + 0.5 * lm, cells[k + 1] - 0.5 * lm
        t[b] = np.sort(lo + rng.uniform(0, 1, N) * (hi - lo))
        f = 0.8 * np.sin(t[b] / (2.0 * lm) + b) + 0.3 * rng.normal(size=N)
        if lik_kind == "poisson":
            y[b] = rng.poisson(np.exp(f))
        else:
            y[b] = f + 0.3 * rng.normal(size=N) if lik_kind == "gaussian" else (f > 0)
    gone = rng.uniform(size=(B, N)) < absent
    gone[:, 0] = False
    y[gone] = np.nan
    return z, t, y


def fd_gradient(spec, jitter, z, t, y, lik, n1, n2, rel_step=1e-6):
    """Central differences of sum_b (dense np.longdouble ELBO of series b at its sites) in each leaf: the yardstick."""
    return sum(S.fd_gradient(spec, jitter, z, tb, yb, lik, a, b, rel_step) for (tb, yb), a, b in zip(present(t, y), n1, n2))


def pair_moments(mu, Sig, Sub, P0, dtype=np.float64):
    """mu_pair [M + 1, 2d], Sigma_pair [M + 1, 2d, 2d] per interval of ONE chain from its natural marginals mu [M, d], Sig [M, d, d],
    Sub [M, d, d] (Sigma_{t+1,t} at t); the prior (zero mean, P0) pads both ends, zero cross block there."""
    M, d = mu.shape
    mp, Sp = np.zeros((M + 1, 2 * d), dtype=dtype), np.zeros((M + 1, 2 * d, 2 * d), dtype=dtype)
    for m in range(M + 1):
        Sp[m, :d, :d] = Sig[m - 1] if m > 0 else P0
        Sp[m, d:, d:] = Sig[m] if m < M else P0
        if m > 0:
            mp[m, :d] = mu[m - 1]
        if m < M:
            mp[m, d:] = mu[m]
        if 0 < m < M:
            Sp[m, d:, :d], Sp[m, :d, d:] = Sub[m - 1], Sub[m - 1].T
    return mp, Sp


def conditional_score(spec, jitter, z, t, a, b, w, mu, Sig, Sub, P0, dtype=np.longdouble):
    """Per-point contributions [B, N, nterm, 3, 2] of the points t [B, N] (cotangents a, b [B, N], projections w [B, N, 2d]) to the
    (rate, var) score at the natural marginals mu [B, M, d], Sig, Sub [B, M, d, d] of the B chains: np_sparse_hyper.conditional_score
    row by row."""
    M = len(z)
    out = []
    for tb, ab, bb, wb, m, Sg, Sb in zip(t, a, b, w, mu, Sig, Sub):
        idx, glo, ghi = S.gaps(tb, z)
        mp, Sp = pair_moments(m, Sg, Sb, P0, dtype)
        wl = wb.astype(dtype)
        wbar = ab.astype(dtype)[:, None] * mp[idx] + 2.0 * bb.astype(dtype)[:, None] * np.einsum("ijk,ik->ij", Sp[idx], wl)
        out.append(S.conditional_score(spec, jitter, glo, ghi, idx, M, ab, bb, wbar, wl, dtype=dtype))
    return np.stack(out)
