"""
80-bit host reference of the sparse-CVI local kernels (csrc/mfgm_sparse.h, entry points mfgm_sparse_predict[_kl], mfgm_sparse_site_update[_q],
mfgm_cond_predict and mfgm_sparse_theta of include/mfgm.h) and the generator of the inputs the host and GPU tests share.

Plain NumPy restating include/mfgm.h and the header comment of csrc/mfgm_sparse.h, not the kernels' loops.  Every function takes the
float type `ft`: np.longdouble (the reference) or np.float64 (the fp64 twin: the same code, the yardstick of tests/test_host_sparse.py),
and returns next to each output the sum of the absolute values of the terms the output is a sum of: the derived rounding bound of
tests/test_gpu_sparse.py is  4 n EPS sum|terms|.

Conventions (include/mfgm.h): M inducing states, intervals m = 0 .. M; interval m lies between the states m - 1 and m, the prior
(prior_mean, prior_cov) stands in for state -1 and for state M and has no cross covariance with anything.  mu [M, d], Sig [M, d, d],
Sub [M, d, d] with Sub[t] = Cov(x_{t+1}, x_t); Sub[M-1] stands for no pair and holds NaN in the generated cases, as Ps[M-1] does: a
kernel that reads either shows it.  seg [M + 2] are the CSR offsets of the data points per interval.
"""
from types import SimpleNamespace

import numpy as np

from tests.np_cq import LD, EPS  # noqa: F401

COUNT_VALUES = (0, 1, 2, 7, 8, 9, 31, 32, 33, 65)
M1_ALL = (2, 3, 31, 32, 33, 64, 65, 70)     # M + 1: every tail of the groupings 1, 2, 4, 8 (k_sparse_sites) and 4 x 8 (k_sparse_sites_q)
LRS = (0.7, 1.0)
AD, AS = -1.75, 0.6                          # the scalings of Pd and Ps: different, so that one taken for the other shows
ROUND, WG, CHUNK = 4, 32, 32                 # k_sparse_sites_q: sites per round, sites per workgroup, data points per LDS chunk


def _T(x):
    return np.swapaxes(x, -1, -2)


# ---- layouts ------------------------------------------------------------------------------------------------------------------------------------
def pack(nat2, d):
    """[..., 2d, 2d] -> quadrant-packed [..., d (d + 1) + d^2] (include/mfgm.h; the packing of tests/test_gpu_st._pack)."""
    i, j = np.tril_indices(d)
    lead = nat2.shape[:-2]
    return np.concatenate([nat2[..., i, j], nat2[..., d:, :d].reshape(lead + (d * d,)), nat2[..., d + i, d + j]], axis=-1)


def unpack(q, d):
    """The symmetric [..., 2d, 2d] tensor of a quadrant-packed one."""
    i, j = np.tril_indices(d)
    et = len(i)
    out = np.zeros(q.shape[:-1] + (2 * d, 2 * d), dtype=q.dtype)
    out[..., i, j] = q[..., :et]
    out[..., j, i] = q[..., :et]
    ll = q[..., et:et + d * d].reshape(q.shape[:-1] + (d, d))
    out[..., d:, :d] = ll
    out[..., :d, d:] = _T(ll)
    out[..., d + i, d + j] = q[..., et + d * d:]
    out[..., d + j, d + i] = q[..., et + d * d:]
    return out


# ---- counts --------------------------------------------------------------------------------------------------------------------------------------
def counts(M1, rng, ends=True):
    """Data points per interval, placed on purpose (the conditions are asserted by check_counts).  The first sixteen and the sites
    30 .. 34 are fixed, the others drawn from {0, 1, 2, 3}; shorter chains take a prefix.  ends: the first and the last interval hold
    data; otherwise both are empty."""
    fixed = [2, 33, 0, 8, 1, 1, 1, 1, 1, 1, 7, 65, 9, 31, 32, 0]
    cnt = np.concatenate([fixed, rng.choice([0, 1, 2, 3], size=max(70, M1) - len(fixed), p=[0.3, 0.4, 0.2, 0.1])]).astype(np.int64)
    cnt[30:35] = 0
    cnt = cnt[:M1]
    cnt[0], cnt[-1] = (2, 7) if ends else (0, 0)
    return cnt


def check_counts(cnt):
    """The conditions the issue of this suite sets for the full-size case (M + 1 >= 70); returns what was found, for the record."""
    M1 = len(cnt)
    seg = np.concatenate([[0], np.cumsum(cnt)])
    found = SimpleNamespace()
    assert set(COUNT_VALUES) <= set(int(c) for c in cnt), "a required count is missing"
    # a run of >= 5 one-point sites that contains a whole round of four: its 32-point chunk spans four sites
    found.round_of_ones = None
    for m0 in range(0, M1 - ROUND + 1, ROUND):
        if np.all(cnt[m0:m0 + ROUND] == 1):
            lo, hi = m0, m0 + ROUND
            while lo > 0 and cnt[lo - 1] == 1:
                lo -= 1
            while hi < M1 and cnt[hi] == 1:
                hi += 1
            if hi - lo >= 5:
                found.round_of_ones = (lo, hi)
    assert found.round_of_ones is not None, "no run of five one-point sites over a whole round"
    # a site of 65 points that starts inside a chunk of its round and so spans three chunks
    found.long_site = None
    for m in np.nonzero(cnt == 65)[0]:
        off = int(seg[m] - seg[m - m % ROUND])
        if off % CHUNK != 0 and (off + 65 - 1) // CHUNK - off // CHUNK >= 2:
            found.long_site = (int(m), off)
    assert found.long_site is not None, "no 65-point site starting mid-chunk"
    # empty sites on both sides of a workgroup boundary of k_sparse_sites_q (32 sites; also one of every k_sparse_sites grouping)
    assert M1 > WG + 1 and np.all(cnt[WG - 2:WG + 2] == 0), "no run of empty sites across a workgroup boundary"
    return found


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------------
def make_case(d, M1, ends=True, seed=0):
    """Inputs in which no mapping mistake cancels: Sig blocks symmetric and all different, Sub blocks not symmetric, prior_cov different
    from every Sig, non-zero prior_mean, dense w without repeated entries, Pd / Ps not symmetric, g2 of mixed magnitude and sign, old
    sites non-zero and symmetric, nothing negligibly small.  The pair covariances do not come from a chain; their smallest eigenvalue is
    asserted > 0.05 (as tests/test_gpu_st._case does)."""
    rng = np.random.default_rng([d, M1, int(ends), seed])
    n, M = 2 * d, M1 - 1
    A = rng.normal(size=(M1, n, n)) / np.sqrt(n)
    S = A @ _T(A) + 0.5 * np.eye(n)
    Sig = S[:M, d:, d:].copy()
    Sub = np.full((M, d, d), np.nan)
    Sub[:M - 1] = 0.3 * S[1:M, d:, :d]
    P0 = S[M, d:, d:].copy()
    mu = rng.normal(size=(M, d))
    pm = 0.3 + 0.1 * rng.normal(size=d)
    cnt = counts(M1, rng, ends)
    seg = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    N = int(seg[-1])
    away = lambda x, lo: np.sign(x) * (lo + np.abs(x))          # nothing negligibly small
    Ps = away(rng.normal(size=(M, d, d)), 0.1)
    Ps[M - 1] = np.nan
    cs = SimpleNamespace(
        d=d, M=M, M1=M1, N=N, cnt=cnt, seg=seg, idx=np.repeat(np.arange(M1), cnt), mu=mu, Sig=Sig, Sub=Sub, P0=P0, pm=pm,
        w=away(rng.normal(size=(N, n)), 0.2) * (0.6 / np.sqrt(n)), c=rng.uniform(0.05, 0.2, size=N), g1=away(rng.normal(size=N), 0.1),
        g2=-rng.uniform(0.1, 1.0, size=N) * 10.0 ** rng.integers(-2, 2, size=N) * rng.choice([1.0, 1.0, 1.0, -1.0], size=N),
        nat1=away(0.3 * rng.normal(size=(M1, n)), 0.05), nat2=(lambda B: away(-0.5 * (B + _T(B)), 0.1))(rng.normal(size=(M1, n, n))),
        Pd=away(rng.normal(size=(M, d, d)), 0.1), Ps=Ps, mup=rng.normal(size=(M, d)), aD=AD, aS=AS,
        plin=away(rng.normal(size=(M, d)), 0.1), pdiag=away(rng.normal(size=(M, d, d)), 0.1), psub=away(rng.normal(size=(M, d, d)), 0.1))
    PC, _ = pairs(cs, np.float64)
    assert np.linalg.eigvalsh(PC).min() > 0.05
    assert len(np.unique(cs.w)) == cs.w.size
    for x in vars(cs).values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return cs


def make_queries(cs, N, seed=0):
    """Query points of mfgm_cond_predict on the marginals of `cs`: idx unsorted, repeated and (N >= 4) holding 0, 1, M - 1 and M;
    P [N, d, 2d] dense, T [N, d, d] not symmetric (the kernel adds it entry by entry)."""
    rng = np.random.default_rng([cs.d, cs.M1, N, seed, 77])
    d, M = cs.d, cs.M
    idx = rng.integers(0, M + 1, size=N)
    if N >= 4:
        idx[[3, N // 2, 0, N - 1]] = (0, 1, M - 1, M)
        idx[1] = idx[N - 2]                                     # a repeat, apart
        assert np.any(np.diff(idx) < 0) or M < 2
    q = SimpleNamespace(N=N, idx=idx.astype(np.int32), P=rng.normal(size=(N, d, 2 * d)) / np.sqrt(2 * d) + 0.05,
                        T=rng.normal(size=(N, d, d)) + 0.1)
    for x in vars(q).values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return q


def shard(cs, m_lo, m_hi):
    """What the process that owns the intervals [m_lo, m_hi) holds: seg rebased to 0 with m_hi - m_lo + 1 entries, the per-point arrays
    of the owned points only; (seg, slice of the owned points)."""
    i0, i1 = int(cs.seg[m_lo]), int(cs.seg[m_hi])
    return (cs.seg[m_lo:m_hi + 1] - cs.seg[m_lo]).astype(np.int32), slice(i0, i1)


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------------
def pair(cs, m, ft=LD):
    """(PC [2d, 2d], pm [2d]) of interval m: the states m - 1 and m, the prior below interval 0 and above interval M, a zero cross block
    at both ends; lower-left block Cov(x_m, x_{m-1}) = Sub[m - 1], upper-right its transpose."""
    d, M = cs.d, cs.M
    P0, pm0 = np.asarray(cs.P0, dtype=ft), np.asarray(cs.pm, dtype=ft)
    PC, pmu = np.zeros((2 * d, 2 * d), dtype=ft), np.zeros(2 * d, dtype=ft)
    PC[:d, :d], pmu[:d] = (P0, pm0) if m == 0 else (np.asarray(cs.Sig[m - 1], dtype=ft), np.asarray(cs.mu[m - 1], dtype=ft))
    PC[d:, d:], pmu[d:] = (P0, pm0) if m == M else (np.asarray(cs.Sig[m], dtype=ft), np.asarray(cs.mu[m], dtype=ft))
    if 0 < m < M:
        C = np.asarray(cs.Sub[m - 1], dtype=ft)
        PC[d:, :d], PC[:d, d:] = C, C.T
    return PC, pmu


def pairs(cs, ft=LD):
    out = [pair(cs, m, ft) for m in range(cs.M1)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def predict(cs, ft=LD):
    """fmu_i = w_i . pm, fvar_i = c_i + w_i^T PC w_i with the pair of the interval of point i; (fmu, fvar, sum|terms| of each)."""
    PC, pmu = pairs(cs, ft)
    w, c = np.asarray(cs.w, dtype=ft), np.asarray(cs.c, dtype=ft)
    PCi, pmi = PC[cs.idx], pmu[cs.idx]
    fmu = np.sum(w * pmi, axis=-1)
    amu = np.sum(np.abs(w * pmi), axis=-1)
    terms = w[:, :, None] * PCi * w[:, None, :]
    return fmu, c + terms.sum(axis=(-1, -2)), amu, np.abs(c) + np.abs(terms).sum(axis=(-1, -2))


def kl_terms(cs, m_lo=0, m_hi=None, ft=LD):
    """The comment on SparseKl: node m < M gives  aD Pd_m . (Sig_m + dv_m dv_m^T), the pair (m, m - 1), m >= 1, gives
    2 aS Ps_{m-1} . (Sub_{m-1} + dv_m dv_{m-1}^T), dv = mup - mu; the first summands are the trace terms, the second the Mahalanobis
    terms.  Returns per node (tr [M], mh [M], sum|terms| of each [M]) and the sums over the owned nodes [m_lo, min(m_hi, M))."""
    M = cs.M
    m_hi = M + 1 if m_hi is None else m_hi
    c = lambda x: np.asarray(x, dtype=ft)
    Pd, Ps, Sig, Sub, dv, aD, aS = c(cs.Pd), c(cs.Ps), c(cs.Sig), c(cs.Sub), c(cs.mup) - c(cs.mu), ft(cs.aD), ft(cs.aS)
    t_node = aD * Pd * Sig
    m_node = aD * Pd * dv[:, :, None] * dv[:, None, :]
    t_pair, m_pair = np.zeros_like(t_node), np.zeros_like(m_node)
    t_pair[1:] = ft(2) * aS * Ps[:M - 1] * Sub[:M - 1]
    m_pair[1:] = ft(2) * aS * Ps[:M - 1] * dv[1:, :, None] * dv[:M - 1, None, :]
    s = lambda *x: sum(v.sum(axis=(-1, -2)) for v in x)
    tr, mh, atr, amh = s(t_node, t_pair), s(m_node, m_pair), s(np.abs(t_node), np.abs(t_pair)), s(np.abs(m_node), np.abs(m_pair))
    own = slice(m_lo, min(m_hi, M))
    return SimpleNamespace(tr=tr, mh=mh, atr=atr, amh=amh, trace=tr[own].sum(), maha=mh[own].sum(), atrace=atr[own].sum(),
                           amaha=amh[own].sum(), nodes=max(0, min(m_hi, M) - m_lo))


def site_sums(cs, ft=LD):
    """s_m = (sum_i g1_i w_i, sum_i g2_i w_i w_i^T) over the points of interval m, dense [M+1, 2d] and [M+1, 2d, 2d], and the sums of the
    absolute values of their terms."""
    c = lambda x: np.asarray(x, dtype=ft)
    w, g1, g2, n = c(cs.w), c(cs.g1), c(cs.g2), 2 * cs.d
    s1, a1, s2, a2 = (np.zeros((cs.M1, n), dtype=ft), np.zeros((cs.M1, n), dtype=ft), np.zeros((cs.M1, n, n), dtype=ft),
                      np.zeros((cs.M1, n, n), dtype=ft))
    for m in np.nonzero(cs.cnt)[0]:
        sl = slice(cs.seg[m], cs.seg[m + 1])
        t1 = g1[sl, None] * w[sl]
        t2 = g2[sl, None, None] * w[sl, :, None] * w[sl, None, :]
        s1[m], a1[m], s2[m], a2[m] = t1.sum(0), np.abs(t1).sum(0), t2.sum(0), np.abs(t2).sum(0)
    return s1, s2, a1, a2


def site_update(cs, lr, ft=LD, sums=None):
    """sites <- (1 - lr) sites + lr s over the points of each interval, dense [M+1, 2d, 2d]; (nat1, nat2, sum|terms| of each).
    (1 - lr) is formed in fp64, as the entry point receives lr as a double.  sums: site_sums(cs, ft), when the caller keeps them."""
    s1, s2, a1, a2 = site_sums(cs, ft) if sums is None else sums
    o1, o2 = np.asarray(cs.nat1, dtype=ft), np.asarray(cs.nat2, dtype=ft)
    keep, lr = ft(1.0 - lr), ft(lr)
    return keep * o1 + lr * s1, keep * o2 + lr * s2, np.abs(keep * o1) + lr * a1, np.abs(keep * o2) + lr * a2


def cond_predict(cs, q, ft=LD):
    """mean_i = P_i pm, cov_i = T_i + P_i PC P_i^T with the pair of interval idx_i; (mean, cov, sum|terms| of each)."""
    PC, pmu = pairs(cs, ft)
    P, T = np.asarray(q.P, dtype=ft), np.asarray(q.T, dtype=ft)
    PCi, pmi = PC[q.idx], pmu[q.idx]
    tm = P * pmi[:, None, :]
    cov = T + np.einsum("nik,nkl,njl->nij", P, PCi, P)
    acov = np.abs(T) + np.einsum("nik,nkl,njl->nij", np.abs(P), np.abs(PCi), np.abs(P))
    return tm.sum(-1), cov, np.abs(tm).sum(-1), acov


def theta(cs, T, with_plin=True, ft=LD):
    """Posterior naturals of the first T inducing states: site t + 1 starts at state t, site t ends there; sub_t takes twice the
    lower-left block of site t + 1 and is exactly zero at the last node.  (lin, diag, sub, sum|terms| of each)."""
    d = cs.d
    c = lambda x: np.asarray(x, dtype=ft)
    n1, n2, plin, pdiag, psub = c(cs.nat1), c(cs.nat2), c(cs.plin[:T]), c(cs.pdiag[:T]), c(cs.psub[:T])
    if not with_plin:
        plin = np.zeros_like(plin)
    terms_l = (plin, n1[1:T + 1, :d], n1[:T, d:])
    terms_d = (pdiag, n2[1:T + 1, :d, :d], n2[:T, d:, d:])
    terms_s = (psub, ft(2) * n2[1:T + 1, d:, :d])
    last = np.ones((T, 1, 1), dtype=ft)
    last[T - 1] = 0
    s = lambda ts: sum(ts)
    a = lambda ts: sum(np.abs(t) for t in ts)
    return s(terms_l), s(terms_d), s(terms_s) * last, a(terms_l), a(terms_d), a(terms_s) * last


# ---- the bound ---------------------------------------------------------------------------------------------------------------------------------------
def ratio(got, want, absterms, n):
    """max |got - want| / (4 n EPS sum|terms|) over the entries; entries whose bound is 0 must be equal and count as 0.  n may be an
    array (per entry)."""
    got, want, absterms = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD), np.asarray(absterms, dtype=LD)
    assert got.shape == want.shape == absterms.shape, (got.shape, want.shape, absterms.shape)
    if got.size == 0:
        return 0.0
    assert np.all(np.isfinite(got))
    bound = 4 * np.broadcast_to(np.asarray(n, dtype=LD), got.shape) * EPS * absterms
    err = np.abs(got - want)
    zero = bound == 0
    assert np.all(err[zero] == 0), "an entry with a zero bound differs"
    return float(np.max(np.where(zero, 0, err / np.where(zero, 1, bound))))
