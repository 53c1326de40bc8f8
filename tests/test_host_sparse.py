"""
Host tests (no GPU) of tests/np_sparse.py, the 80-bit reference and input generator of tests/test_gpu_sparse.py: the fp64 twin stays far
inside the derived bound 4 n EPS sum|terms| on every case (the yardstick tests/test_gpu_sparse.py cites), the reference agrees with
an independent dense construction on a genuine chain (the joint covariance of all inducing states assembled from oracle/np_btd and
projected), the quadrant-packed layout round-trips, and the generator's count patterns and shard slicing are what the GPU tests rely on.
"""
import numpy as np
import pytest

from oracle import np_btd
from tests import np_sparse
from tests.helpers import random_spd_btd
from tests.np_sparse import LD

DIMS = list(range(1, 33))


@pytest.mark.parametrize("d", DIMS)
def test_twin_is_far_inside_the_bound(d):
    """The reference's code in fp64 against itself in 80-bit, every output, over the full-size case and the two shortest chains: the
    twin's error over the bound is the yardstick, and has to be well below 1 for the bound to mean anything on these inputs."""
    worst = {}

    def note(name, r):
        worst[name] = max(worst.get(name, 0.0), r)

    for M1, ends in ((70, True), (70, False), (2, True), (3, True)):
        cs = np_sparse.make_case(d, M1, ends)
        n2 = 2 * d
        want, twin = np_sparse.predict(cs), np_sparse.predict(cs, np.float64)
        note("fmu", np_sparse.ratio(twin[0], want[0], want[2], n2))
        note("fvar", np_sparse.ratio(twin[1], want[1], want[3], n2 * n2 + 1))
        kw, kt = np_sparse.kl_terms(cs), np_sparse.kl_terms(cs, ft=np.float64)
        note("trace", np_sparse.ratio(kt.trace, kw.trace, kw.atrace, 2 * d * d * kw.nodes))
        note("maha", np_sparse.ratio(kt.maha, kw.maha, kw.amaha, 2 * d * d * kw.nodes))
        for lr in np_sparse.LRS:
            want, twin = np_sparse.site_update(cs, lr), np_sparse.site_update(cs, lr, np.float64)
            n = cs.cnt + 1
            note("nat1", np_sparse.ratio(twin[0], want[0], want[2], n[:, None]))
            note("nat2", np_sparse.ratio(twin[1], want[1], want[3], n[:, None, None]))
        q = np_sparse.make_queries(cs, 40)
        want, twin = np_sparse.cond_predict(cs, q), np_sparse.cond_predict(cs, q, np.float64)
        note("cond mean", np_sparse.ratio(twin[0], want[0], want[2], n2))
        note("cond cov", np_sparse.ratio(twin[1], want[1], want[3], n2 * n2 + 1))
        want, twin = np_sparse.theta(cs, cs.M), np_sparse.theta(cs, cs.M, ft=np.float64)
        for k, name in enumerate(("lin", "diag", "sub")):
            note("theta " + name, np_sparse.ratio(twin[k], want[k], want[3 + k], 3))
    print(f"  d={d} twin error / bound: " + "  ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert max(worst.values()) < 0.25, worst


def _chain(rng, M, d):
    """A genuine chain: (mu, Sig, Sub, the dense joint covariance of its M states) from a random block-tri-diagonal precision."""
    diag, sub, _, _ = random_spd_btd(rng, (), M, d)
    Ld, Ls = np_btd.cholesky(diag, sub)
    Sig, Sub = np_btd.inverse_blocks(Ld, Ls)
    J = np.linalg.inv(np_btd.to_dense(diag, sub))
    return rng.normal(size=(M, d)), Sig, (np.zeros((M, d, d)) if Sub is None else np.concatenate([Sub, np.full((1, d, d), np.nan)])), J


@pytest.mark.parametrize("d,M", [(1, 5), (3, 1), (3, 2), (3, 6), (4, 5)])
def test_reference_against_the_dense_joint(d, M):
    """predict, cond_predict and kl_terms on a genuine chain against the joint N(mean, J) of the states (-1: prior, 0 .. M-1, M: prior)
    assembled densely: a data point of interval m sees the joint through the selection of the states m - 1 and m."""
    rng = np.random.default_rng([d, M])
    cs0 = np_sparse.make_case(d, M + 1)
    mu, Sig, Sub, J = _chain(rng, M, d)
    Sub = Sub if M > 1 else np.full((1, d, d), np.nan)
    cs = np_sparse.SimpleNamespace(**{**vars(cs0), "mu": mu, "Sig": Sig, "Sub": Sub})
    n = (M + 2) * d
    Jx, mx = np.zeros((n, n)), np.concatenate([cs.pm, mu.reshape(-1), cs.pm])
    Jx[:d, :d], Jx[d:-d, d:-d], Jx[-d:, -d:] = cs.P0, J, cs.P0
    fmu, fvar, _, _ = np_sparse.predict(cs)
    q = np_sparse.make_queries(cs, 12)
    cm, cc, _, _ = np_sparse.cond_predict(cs, q)
    for i in range(cs.N):
        E = np.zeros((2 * d, n))
        E[:, cs.idx[i] * d:(cs.idx[i] + 2) * d] = np.eye(2 * d)
        v = cs.w[i] @ E
        np.testing.assert_allclose(float(fmu[i]), v @ mx, rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(float(fvar[i]), cs.c[i] + v @ Jx @ v, rtol=1e-12, atol=1e-13)
    for i in range(q.N):
        E = np.zeros((2 * d, n))
        E[:, q.idx[i] * d:(q.idx[i] + 2) * d] = np.eye(2 * d)
        V = q.P[i] @ E
        np.testing.assert_allclose(cm[i].astype(np.float64), V @ mx, rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(cc[i].astype(np.float64), q.T[i] + V @ Jx @ V.T, rtol=1e-12, atol=1e-12)
    # KL terms: the full precision-like matrix with aD Pd on the diagonal and aS Ps below it (its transpose above), dotted with J + dv dv^T
    Pf = np_btd.to_dense(cs.aD * cs.Pd, cs.aS * np.nan_to_num(cs.Ps[:M - 1]) if M > 1 else None)
    dv = (cs.mup - mu).reshape(-1)
    band = np_btd.to_dense(np.ones((M, d, d)), np.ones((M - 1, d, d)) if M > 1 else None)       # J is dense; KL reads its band only
    kl = np_sparse.kl_terms(cs)
    np.testing.assert_allclose(float(kl.trace), np.sum(Pf * J * band), rtol=1e-12)
    np.testing.assert_allclose(float(kl.maha), dv @ Pf @ dv, rtol=1e-12)
    # ownership: the sums over complementary shards add up to the whole
    k = max(1, M // 2)
    a, b = np_sparse.kl_terms(cs, 0, k), np_sparse.kl_terms(cs, k, M + 1)
    assert a.nodes + b.nodes == M
    np.testing.assert_allclose(float(a.trace + b.trace), float(kl.trace), rtol=1e-15)


@pytest.mark.parametrize("d", [1, 2, 5, 16])
def test_packed_layout_round_trip(d):
    """pack keeps d (d + 1) + d^2 entries of a symmetric [2d, 2d] site -- upper-left lower triangle, lower-left block in full,
    lower-right lower triangle -- and unpack restores the site; entry positions as include/mfgm.h states them."""
    rng = np.random.default_rng(d)
    B = rng.normal(size=(3, 2 * d, 2 * d))
    S = B + np.swapaxes(B, -1, -2)
    q = np_sparse.pack(S, d)
    et = d * (d + 1) // 2
    assert q.shape == (3, 2 * et + d * d)
    assert np.array_equal(np_sparse.unpack(q, d), S)
    assert q[1, 0] == S[1, 0, 0] and q[1, et - 1] == S[1, d - 1, d - 1]
    assert q[1, et] == S[1, d, 0] and q[1, et + d * d - 1] == S[1, 2 * d - 1, d - 1]
    assert q[1, et + d * d] == S[1, d, d] and q[1, -1] == S[1, 2 * d - 1, 2 * d - 1]
    if d > 1:
        assert q[1, 1] == S[1, 1, 0] and q[1, et + 1] == S[1, d, 1] and q[1, et + d] == S[1, d + 1, 0]


@pytest.mark.parametrize("ends", [True, False])
def test_generator_count_conditions(ends):
    """Every required count occurs, the ends are populated (or both empty), a whole round of four one-point sites lies in a run of at
    least five, a 65-point site starts mid-chunk and spans three chunks, empty sites cross a workgroup boundary; the inputs are what
    make_case promises."""
    for d in (1, 16, 31):
        cs = np_sparse.make_case(d, 70, ends)
        found = np_sparse.check_counts(cs.cnt)
        print(f"  d={d} ends={ends}: N={cs.N}, one-point run {found.round_of_ones}, 65-point site (index, offset in its round) {found.long_site}")
        assert (cs.cnt[0] > 0 and cs.cnt[-1] > 0) if ends else (cs.cnt[0] == 0 and cs.cnt[-1] == 0)
        assert cs.N <= 600 and cs.seg[-1] == cs.N and len(cs.seg) == cs.M + 2
        assert np.array_equal(cs.Sig, np.swapaxes(cs.Sig, -1, -2)) and np.array_equal(cs.nat2, np.swapaxes(cs.nat2, -1, -2))
        if d > 1:
            assert not np.any(np.isclose(cs.Sub[:-1], np.swapaxes(cs.Sub[:-1], -1, -2)).all(axis=(-1, -2)))
            assert not np.allclose(cs.Pd, np.swapaxes(cs.Pd, -1, -2)) and not np.allclose(cs.Ps[:-1], np.swapaxes(cs.Ps[:-1], -1, -2))
        assert np.all(np.isnan(cs.Sub[-1])) and np.all(np.isnan(cs.Ps[-1]))
        assert len({cs.Sig[m].tobytes() for m in range(cs.M)} | {cs.P0.tobytes()}) == cs.M + 1
        assert np.all(cs.pm != 0) and np.abs(cs.g2).max() / np.abs(cs.g2).min() > 100
        for name in ("w", "g1", "g2", "nat1", "nat2", "Pd", "pdiag"):
            assert np.abs(getattr(cs, name)).min() > 1e-4, name
    for M1 in np_sparse.M1_ALL:
        cs = np_sparse.make_case(3, M1, True)
        assert len(cs.cnt) == M1 and cs.cnt[0] > 0 and cs.cnt[-1] > 0


@pytest.mark.parametrize("m_lo,m_hi", [(0, 11), (11, 70), (11, 12), (9, 46), (30, 34)])
def test_shard_slicing(m_lo, m_hi):
    """The owned points are one contiguous slice of the sorted data, seg is rebased to 0 and has m_hi - m_lo + 1 entries."""
    cs = np_sparse.make_case(3, 70)
    seg, own = np_sparse.shard(cs, m_lo, m_hi)
    assert seg[0] == 0 and len(seg) == m_hi - m_lo + 1 and seg.dtype == np.int32
    assert np.array_equal(np.diff(seg), cs.cnt[m_lo:m_hi])
    assert np.array_equal(np.arange(cs.N)[own], np.nonzero((cs.idx >= m_lo) & (cs.idx < m_hi))[0])
    assert seg[-1] == own.stop - own.start
