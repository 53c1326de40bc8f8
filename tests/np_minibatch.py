"""
NumPy restatement of mini-batch sparse CVI (include/mfgm.h, mfgm_sparse_batch_predict_lik / mfgm_sparse_batch_seg;
SparseCVIGaussianProcess(num_data=)); not a test module.  Built on tests/np_sparse_hyper: `gaps`, `conditional_stats`, `ve_and_grads`
and the dense `SparseChain`.  Any dtype (np.longdouble is the yardstick of tests/test_gpu_minibatch.py); the Bernoulli rule is
tests/np_lik's, in fp64.

  batch_pass   the contract of mfgm_sparse_batch_predict_lik on time points in any order, with the sum of the absolute terms of every
               output next to it (what an error is measured against)
  batch_seg    the contract of mfgm_sparse_batch_seg
  BatchChain   the model on one batch: SparseChain with the expectation term and the site gradients weighed by num_data / n and an
               optional mean function
"""
import numpy as np

from tests import np_hyper as H
from tests import np_lik
from tests import np_sparse_hyper as S


def batch_rows(spec, jitter, z, t, dtype=np.longdouble):
    """(idx [n], w [n, 2d], c [n]) of time points in any order; a non-finite time has idx = 0 and a zero row."""
    t = np.asarray(t, dtype=np.float64)
    n, d = len(t), H.state_dim(spec)
    fin = np.isfinite(t)
    idx, w, c = np.zeros(n, dtype=np.int64), np.zeros((n, 2 * d), dtype=dtype), np.zeros(n, dtype=dtype)
    if fin.any():
        idx[fin], lo, hi = S.gaps(t[fin], np.asarray(z, dtype=np.float64))
        w[fin], c[fin] = S.conditional_stats(spec, jitter, lo, hi, dtype)
    return idx, w, c


def pair_moments(mu, Sig, Sub, prior_mean, prior_cov, dtype=np.longdouble):
    """mp [M + 1, 2d], Sp [M + 1, 2d, 2d] from the chain marginals mu [M, d], Sig [M, d, d], Sub [M, d, d] (Sigma_{t+1,t} at t): the
    prior's initial state at m = 0 and m = M, a zero cross block there (mfgm_sparse_predict)."""
    M, d = mu.shape
    mp, Sp = np.zeros((M + 1, 2 * d), dtype=dtype), np.zeros((M + 1, 2 * d, 2 * d), dtype=dtype)
    for m in range(M + 1):
        Sp[m, :d, :d] = Sig[m - 1] if m > 0 else prior_cov
        Sp[m, d:, d:] = Sig[m] if m < M else prior_cov
        mp[m, :d] = mu[m - 1] if m > 0 else prior_mean
        mp[m, d:] = mu[m] if m < M else prior_mean
        if 0 < m < M:
            Sp[m, d:, :d], Sp[m, :d, d:] = Sub[m - 1], Sub[m - 1].T
    return mp, Sp


def lik_terms(lik, fmu, fvar, y):
    """(ve, d ve / d fmu, d ve / d fvar, dict of the sums of the absolute terms of the three) of ("gaussian", variance),
    ("poisson", binsize) or ("bernoulli", jitter) per point, in the dtype of fmu (Bernoulli: fp64)."""
    kind, prm = lik
    if kind == "bernoulli":
        f64 = lambda a: np.asarray(a, dtype=np.float64)
        ve, dmu, dv, sc = np_lik.Bernoulli(prm).ve_and_grads(f64(fmu), f64(fvar), f64(y))
        return ve, dmu, dv, sc
    ve, dmu, dv = S.ve_and_grads(lik, fmu, fvar, y)
    dtype = fmu.dtype.type
    if kind == "gaussian":
        v = dtype(prm)
        sc = dict(ve=np.abs(0.5 * np.log(2 * dtype(np.pi) * v)) + 0.5 * ((y - fmu) ** 2 + np.abs(fvar)) / v,
                  dmu=(np.abs(y) + np.abs(fmu)) / v, dv=0.5 / v * np.ones_like(fmu))
    else:
        e = dtype(prm) * np.exp(fmu + 0.5 * fvar)
        sc = dict(ve=np.abs(y * np.log(dtype(prm))) + np.abs(y * fmu) + e + np.abs(y * fmu - e - ve + y * np.log(dtype(prm))),
                  dmu=np.abs(y) + e, dv=0.5 * e)
    return ve, dmu, dv, sc


def batch_pass(spec, jitter, z, t, mu, Sig, Sub, prior_mean, prior_cov, lik=None, y=None, scale=1.0, shift=None, dtype=np.longdouble):
    """The outputs of mfgm_sparse_batch_predict_lik as a dict: idx, w, c, fmu, fvar and, with a likelihood, ve, g1, g2, ve_sum; under
    "scale" the sum of the absolute terms of each of fmu, fvar, ve, g1, g2, ve_sum.  A NaN observation and a non-finite time give
    ve = g1 = g2 = 0; a non-finite time also fmu = shift, fvar = 0."""
    cast = lambda a: np.asarray(a, dtype=dtype)
    idx, w, c = batch_rows(spec, jitter, z, t, dtype)
    mp, Sp = pair_moments(cast(mu), cast(Sig), cast(Sub), cast(prior_mean), cast(prior_cov), dtype)
    n = len(idx)
    sh = np.zeros(n, dtype=dtype) if shift is None else cast(shift)
    g = np.einsum("ij,ij->i", w, mp[idx])
    quad = np.einsum("ij,ijk,ik->ijk", w, Sp[idx], w)
    out = dict(idx=idx, w=w, c=c, fmu=g + sh, fvar=c + quad.sum((1, 2)))
    sc = dict(fmu=np.abs(w * mp[idx]).sum(1) + np.abs(sh), fvar=np.abs(c) + np.abs(quad).sum((1, 2)))
    if lik is not None:
        y = cast(y)
        on = np.isfinite(np.asarray(t, dtype=np.float64)) & ~np.isnan(np.asarray(y, dtype=np.float64))
        ve, g1, g2 = (np.zeros(n, dtype=dtype) for _ in range(3))
        sve, s1, s2 = (np.zeros(n, dtype=dtype) for _ in range(3))
        if on.any():
            e, dmu, dv, ls = lik_terms(lik, out["fmu"][on], out["fvar"][on], y[on])
            s = dtype(scale)
            ve[on], g1[on], g2[on] = s * e, s * (dmu - 2.0 * dv * g[on]), s * dv
            sve[on], s1[on], s2[on] = s * ls["ve"], s * (ls["dmu"] + 2.0 * ls["dv"] * np.abs(g[on])), s * ls["dv"]
        out.update(ve=ve, g1=g1, g2=g2, ve_sum=ve.sum())
        sc.update(ve=sve, g1=s1, g2=s2, ve_sum=sve.sum())
    out["scale"] = sc
    return out


def batch_seg(z, t_sorted):
    """seg [M + 2] of a batch sorted in time: seg[0] = 0, seg[m + 1] = #{t_i <= z_m}, seg[M + 1] = n."""
    t = np.asarray(t_sorted, dtype=np.float64)
    return np.concatenate([[0], np.searchsorted(t, np.asarray(z, dtype=np.float64), side="right"), [len(t)]]).astype(np.int32)


class BatchChain(S.SparseChain):
    """SparseChain on ONE batch (t [n] in any order, y [n]) of a data set of num_data points: scale = num_data / n weighs the
    expectation term of the bound and the site gradients; mean(t) (a callable, or None) shifts the likelihood's mean, the sites stay on
    the zero-mean part."""

    def __init__(self, spec, jitter, z, t, y, lik, num_data, mean=None, dtype=np.float64):
        super().__init__(spec, jitter, z, t, y, lik, dtype=dtype)
        self.scale = dtype(num_data) / dtype(len(self.t))
        self.shift = np.zeros(len(self.t), dtype=dtype) if mean is None else np.asarray(mean(self.t), dtype=dtype)

    def _lik(self, fmu, fvar):
        ve, dmu, dv, _ = lik_terms(self.lik, fmu + self.shift, fvar, self.y)
        return ve, dmu, dv

    def elbo(self, n1, n2):
        mu, Sigma = self.posterior(n1, n2)
        fmu, fvar, _, _ = self.predict(mu, Sigma)
        n = self.M * self.d
        kl = 0.5 * ((self.Lam_p * Sigma).sum() + mu @ self.Lam_p @ mu - n + S.logdet(self.K) - S.logdet(Sigma))
        return self.scale * self._lik(fmu, fvar)[0].sum() - kl

    def update_sites(self, n1, n2, lr):
        mu, Sigma = self.posterior(n1, n2)
        fmu, fvar, _, _ = self.predict(mu, Sigma)
        _, a, b = self._lik(fmu, fvar)
        g1, g2 = self.scale * (a - 2.0 * b * fmu), self.scale * b
        t1, t2 = self.zero_sites()
        for i in range(self.N):
            t1[self.idx[i]] += g1[i] * self.w[i]
            t2[self.idx[i]] += g2[i] * np.outer(self.w[i], self.w[i])
        return (1 - lr) * n1 + lr * t1, (1 - lr) * n2 + lr * t2
