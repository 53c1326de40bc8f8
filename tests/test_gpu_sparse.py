"""
GPU tests of the sparse-CVI local kernels (csrc/mfgm_sparse.h, launched from csrc/mfgm_api_sparse.hip) against the 80-bit host reference
tests/np_sparse.py, through the C ABI, at every state dimension d = 1 ... 32, on inputs in which no mapping mistake cancels
(np_sparse.make_case) and per-interval counts placed on purpose (np_sparse.counts: every count of {0, 1, 2, 7, 8, 9, 31, 32, 33, 65}, a
whole round of four one-point sites, a 65-point site over three LDS chunks, empty sites across a workgroup boundary, both ends populated
or both empty), at M + 1 in {2, 3, 31, 32, 33, 64, 65, 70}.  Sub[M-1] and Ps[M-1], which stand for no pair, hold NaN; outputs are
pre-filled with a sentinel.

Tolerance rule (that of tests/test_gpu_st.py).  Every output is a sum of products of the inputs: with n terms and a handful of roundings
each, |got - want| <= 4 n EPS sum|terms| whatever the order of summation; want and sum|terms| come from the 80-bit reference.  n = 2d
(fmu, the mean of cond_predict), (2d)^2 + 1 (fvar, cov), 2 d^2 x owned nodes (trace, maha), points of the site + 1 (a site entry), 3
(theta).  Entries whose bound is 0 are compared exactly; no entry is skipped.  Every check prints err / bound.

Instantiations the dispatch of csrc/mfgm_api_sparse.hip can launch, and the test that launches them:
  k_sparse_predict<2, 8, 16, 32, 64>       odd d = 1 | 3 | 5, 7 | 9 ... 15 | 17 ... 31 test_predict (the KL branch at d >= 9: <32>, <64>)
  k_sparse_predict<4 ... 64> at even d     d = 2 | 4 | 6, 8 | 10 ... 16 | 18 ... 32, MFGM_SPARSE_PREDICT_V=0 (<4> runs at d = 2 only)
                                                                                      test_predict_fallback_route_in_a_child
  k_sparse_predict_v<2>, <8>               even d = 2 ... 16 | 18 ... 32               test_predict, test_shards (d = 12, 16, 32)
  k_sum_partials on kl.part + m_lo                                                    test_predict, test_shards
  k_sparse_sites<1, 2, 4, 8>               d <= 11 | 12 ... 16 | 17 ... 22 | 23 ... 32 test_site_update, test_shards
  k_sparse_sites_q<1, 2, 3, 4, 8, 9>       d <= 11 | 12 ... 15 | 16 ... 19 | 20 ... 22 | 23 ... 31 | 32   test_site_update, test_shards
  k_cond_predict                           d = 1 ... 32 (66 048 B of LDS at d = 32)    test_cond_predict
  k_sparse_theta                           d = 1 ... 32, plin given and NULL           test_theta
  NOT launched: the KL branch of k_sparse_predict<2 ... 16> and of k_sparse_predict_v at d <= 8: mfgm_sparse_predict_kl takes a wide
  plan (8 < d <= 32) and refuses any other, which test_predict asserts at every d <= 8.  (NE = ceil((2 d^2 + d) / 256): d = 11 is
  still NE = 1 with 253 packed entries, and 5, 6, 7 fold to 8 at d = 23 ... 31.)

Largest err / bound measured on an MI355X over every d, case and output of a test (a test passes when <= 1), next to the fp64 twin's
(tests/test_host_sparse.py: the reference's own code in fp64, at most 0.18, on the site entries):
  test_predict                              0.098  (fmu, d = 1, both ends empty); fvar, trace and maha at most 0.01
  test_predict_fallback_route_in_a_child    0.066  (fmu, d = 2)
  test_site_update                          0.136  (nat2); dense and packed sites bit-identical at every d, M + 1 and lr
  test_shards                               0.120  (nat2, d = 12 ... 32); predictions and sites of a shard bit-identical to the whole
  test_cond_predict                         0.078  (mean, d = 1, M = 2)
  test_theta                                0.076  (lin, d = 28, T = 37)
k_cond_predict at d = 32: the runtime accepts the 66 048 B of dynamic LDS on gfx950 (160 KiB per workgroup) and the result holds the
bound; the 65 536 B limit of mfgm_api_fa.hip / mfgm_api_ml.hip is those entry points' own.

What these tests found.  k_sparse_sites summed entry (r, c) of a dense site as (g w_r) w_c, which is rounded otherwise than the
(g w_c) w_r of entry (c, r): the [2d, 2d] site of mfgm_sparse_site_update came out unsymmetric in the last bit at every d (every case of
test_site_update and test_shards failed "symmetric to the bit"), and differed in the last bit from the quadrant-packed site of
mfgm_sparse_site_update_q on the same data.  Fixed in csrc/mfgm_sparse.h: both triangles take (g w_max(r,c)) w_min(r,c), the packed
kernel's rounding; test_site_update now also holds dense == unpack(packed) bit for bit.

Checked once with three deliberately wrong scratch builds of the library (not committed; arithmetic only, no address or bound changed).
(a) the cross block read untransposed in k_sparse_predict and cc paired with the wrong half of w in k_sparse_predict_v: test_predict
fails at every d >= 2 (d = 1 passes: a 1 x 1 block is its own transpose), test_shards at all five d, and the child of the fallback
route.  (b) p1 of k_sparse_sites_q taken from segv[gi]: test_site_update fails at all 32 d, test_shards at all five.  (c) the factor 2
on aS dropped in both predict kernels: test_predict fails at every d >= 9 (the d with a KL pass), test_shards at d = 12, 16, 23, 32,
and the child.  The older tests that reach these kernels were run against the same builds and did not all pass: the side comparisons
of tests/test_gpu_st.py (d in {9, 10, 16, 30, 32}), test_sparse_cvi_d16 and test_sparse_cvi_and_posterior[m32sum] see (a), (b) or (c)
at the d they run; nothing before this suite ran these kernels entry by entry at the other d, on a shard, or through the fallback route.
"""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import np_sparse

pytestmark = pytest.mark.gpu

DIMS = list(range(1, 33))
SHARD_DIMS = [3, 12, 16, 23, 32]
SENT = -7.0e77            # sentinel the outputs are pre-filled with
PAD = 8                   # sentinel entries behind every per-point output
PREDICT_CASES = ((70, True), (70, False), (2, True), (3, True))       # (M + 1, ends populated): the full-size pair, M = 1, M = 2
SITE_CASES = tuple((M1, True) for M1 in np_sparse.M1_ALL) + ((70, False),)
WORST = {}


@pytest.fixture(scope="module")
def amd():
    import torch
    import vidp_amd
    assert torch.cuda.is_available()
    vidp_amd._lib.load()
    return vidp_amd


def dev(x, dtype=np.float64):
    import torch
    return torch.from_numpy(np.array(x, dtype=dtype, order="C")).cuda()          # a copy: the cases are read-only


def host(x):
    return x.detach().cpu().numpy()


def sent(*shape):
    import torch
    return torch.full(shape, SENT, dtype=torch.float64, device="cuda")


def held(test, name, got, want, absterms, n):
    """The bound of the module docstring: |got - want| <= 4 n EPS sum|terms| entry by entry, entries with a zero bound exactly."""
    r = np_sparse.ratio(got, want, absterms, n)
    WORST[test] = max(WORST.get(test, 0.0), r)
    print(f"  {test} {name}: err / bound {r:.4f}  (largest so far in this test {WORST[test]:.4f})")
    assert r <= 1.0, (test, name, r)


# ---- references, computed once and shared ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(d, M1, ends=True):
    return np_sparse.make_case(d, M1, ends)


@functools.lru_cache(maxsize=None)
def ref_predict(d, M1, ends):
    return np_sparse.predict(case(d, M1, ends))


@functools.lru_cache(maxsize=None)
def ref_sums(d, M1, ends):
    return np_sparse.site_sums(case(d, M1, ends))


@functools.lru_cache(maxsize=None)
def ref_sites(d, M1, ends, lr):
    return np_sparse.site_update(case(d, M1, ends), lr, sums=ref_sums(d, M1, ends))


# ---- device side --------------------------------------------------------------------------------------------------------------------------------------
class Dev:
    """The device arrays of a case (of the intervals [m_lo, m_hi) when sharded: per-point arrays of the owned points only, seg rebased)
    and the calls of the C ABI."""

    def __init__(self, amd, cs, own=None, empty=False):
        import torch
        from vidp_amd import _lib
        from vidp_amd.packed import _ptr, _stream
        self.torch, self._ptr, self._stream, self.amd = torch, _ptr, _stream, amd
        self.lib, self.cs = _lib.load(), cs
        self.m_lo, self.m_hi = own if own else (0, cs.M1)
        seg, pts = np_sparse.shard(cs, self.m_lo, self.m_hi)
        if empty:                       # N = 0: no per-point array at all
            seg, pts = np.zeros_like(seg), slice(0, 0)
        self.pts, self.N = pts, int(seg[-1])
        self.keep = dict(seg=dev(seg, np.int32), pm=dev(cs.pm), P0=dev(cs.P0), mu=dev(cs.mu), Sig=dev(cs.Sig), Sub=dev(cs.Sub), Pd=dev(cs.Pd),
                         Ps=dev(cs.Ps), mup=dev(cs.mup))
        if not empty:
            self.keep.update(w=dev(cs.w[pts]), c=dev(cs.c[pts]), g1=dev(cs.g1[pts]), g2=dev(cs.g2[pts]))
        k = self.keep
        sd = self.sd = _lib.SparseData()
        sd.M, sd.d, sd.N = cs.M, cs.d, self.N
        sd.m_lo, sd.m_hi = (self.m_lo, self.m_hi) if own else (0, 0)
        sd.seg, sd.prior_mean, sd.prior_cov = k["seg"].data_ptr(), k["pm"].data_ptr(), k["P0"].data_ptr()
        sd.w, sd.c = (None, None) if empty else (k["w"].data_ptr(), k["c"].data_ptr())

    def predict(self, plan=None):
        """(rc, fmu [N], fvar [N], trace, maha): mfgm_sparse_predict, or mfgm_sparse_predict_kl on `plan`; whatever lies behind the N
        entries must still hold the sentinel."""
        k, p = self.keep, self._ptr
        out, kt = sent(2, self.N + PAD), sent(2)
        if plan is None:
            rc = self.lib.mfgm_sparse_predict(ctypes.byref(self.sd), p(k["mu"]), p(k["Sig"]), p(k["Sub"]), p(out[0]), p(out[1]), self._stream())
        else:
            rc = self.lib.mfgm_sparse_predict_kl(ctypes.byref(self.sd), p(k["mu"]), p(k["Sig"]), p(k["Sub"]), p(out[0]), p(out[1]), plan.h,
                                                 p(k["Pd"]), p(k["Ps"]), self.cs.aD, self.cs.aS, p(k["mup"]), p(kt[0:1]), p(kt[1:2]),
                                                 p(plan.ws), self._stream())
        self.torch.cuda.synchronize()
        o, kt = host(out), host(kt)
        assert np.all(o[:, self.N:] == SENT), "written behind the last data point"
        return rc, o[0, :self.N], o[1, :self.N], kt[0], kt[1]

    def update(self, lr, packed, nat1=None, nat2=None):
        """(rc, nat1 [M+1, 2d], nat2 dense or packed) after mfgm_sparse_site_update[_q] in place; the sites this process does not own are
        pre-filled with the sentinel and must still hold it."""
        cs, p, d = self.cs, self._ptr, self.cs.d
        n1 = np.array(cs.nat1 if nat1 is None else nat1)
        n2 = np.array(cs.nat2 if nat2 is None else nat2)
        n2 = np_sparse.pack(n2, d) if packed else n2
        other = np.ones(cs.M1, dtype=bool)
        other[self.m_lo:self.m_hi] = False
        n1[other], n2[other] = SENT, SENT
        t1, t2 = dev(n1), dev(n2)
        fn = self.lib.mfgm_sparse_site_update_q if packed else self.lib.mfgm_sparse_site_update
        rc = fn(ctypes.byref(self.sd), p(self.keep.get("g1")), p(self.keep.get("g2")), float(lr), p(t1), p(t2), self._stream())
        self.torch.cuda.synchronize()
        o1, o2 = host(t1), host(t2)
        assert np.all(o1[other] == SENT) and np.all(o2[other] == SENT), "a site of another process was written"
        return rc, o1, o2


_PLANS = {}


def plan_of(amd, M, d):
    if (M, d) not in _PLANS:
        _PLANS[(M, d)] = amd.Plan(1, M, d)
    return _PLANS[(M, d)]


def check_predict(test, tag, D, got, d, M1, ends, plan):
    """fmu / fvar of a run (of the shard D owns) against the reference; with a plan also trace and maha over the owned nodes."""
    want = ref_predict(d, M1, ends)
    rc, fmu, fvar, tr, mh = got
    assert rc == 0, (tag, rc)
    held(test, f"{tag} fmu", fmu, want[0][D.pts], want[2][D.pts], 2 * d)
    held(test, f"{tag} fvar", fvar, want[1][D.pts], want[3][D.pts], 4 * d * d + 1)
    if plan is None:
        assert tr == SENT and mh == SENT
    else:
        kl = np_sparse.kl_terms(D.cs, D.m_lo, D.m_hi)
        held(test, f"{tag} trace", tr, kl.trace, kl.atrace, 2 * d * d * kl.nodes)
        held(test, f"{tag} maha", mh, kl.maha, kl.amaha, 2 * d * d * kl.nodes)


@pytest.mark.parametrize("d", DIMS)
def test_predict(amd, d):
    """mfgm_sparse_predict at every d, and mfgm_sparse_predict_kl where the header admits it (a wide plan: d > 8; at d <= 8 it must
    refuse and write nothing), on the two full-size cases, M = 1 and M = 2."""
    test = "test_predict"
    for M1, ends in PREDICT_CASES:
        cs = case(d, M1, ends)
        if M1 == 70:
            np_sparse.check_counts(cs.cnt)
        tag = f"d={d} M+1={M1}{'' if ends else ' empty ends'}"
        D = Dev(amd, cs)
        plain = D.predict()
        check_predict(test, tag, D, plain, d, M1, ends, None)
        again = D.predict()
        assert all(np.array_equal(a, b) for a, b in zip(plain, again)), "two launches differ"
        plan = plan_of(amd, cs.M, d)
        withkl = D.predict(plan)
        if d <= 8:
            assert withkl[0] != 0 and np.all(withkl[1] == SENT) and np.all(withkl[2] == SENT) and withkl[3] == SENT and withkl[4] == SENT
        else:
            check_predict(test, tag + " kl", D, withkl, d, M1, ends, plan)
            assert np.array_equal(withkl[1], plain[1]) and np.array_equal(withkl[2], plain[2]), "the two entry points differ"
            again = D.predict(plan)
            assert all(np.array_equal(a, b) for a, b in zip(withkl, again)), "two launches differ"
        # N = 0, null w and c: the plain entry returns 0 and writes nothing, the _kl entry still gives trace and maha
        E = Dev(amd, cs, empty=True)
        rc, fmu, fvar, tr, mh = E.predict()
        assert rc == 0 and E.N == 0 and tr == SENT and mh == SENT
        if d > 8:
            got = E.predict(plan)
            check_predict(test, tag + " N=0 kl", E, got, d, M1, ends, plan)
            assert got[3] == withkl[3] and got[4] == withkl[4]
        plan.check_info()


def check_sites(test, tag, D, got, d, M1, ends, lr, packed):
    cs = D.cs
    want = ref_sites(d, M1, ends, lr)
    rc, n1, n2 = got
    assert rc == 0, (tag, rc)
    own = slice(D.m_lo, D.m_hi)
    n = (cs.cnt + 1)[own]
    w2, a2 = (np_sparse.pack(want[1], d), np_sparse.pack(want[3], d)) if packed else (want[1], want[3])
    held(test, f"{tag} nat1", n1[own], want[0][own], want[2][own], n[:, None])
    held(test, f"{tag} nat2", n2[own], w2[own], a2[own], n[:, None] if packed else n[:, None, None])
    # sites without data: (1 - lr) old exactly
    empty = np.nonzero(cs.cnt[own] == 0)[0] + D.m_lo
    o2 = np_sparse.pack(np.asarray(cs.nat2), d) if packed else cs.nat2
    assert np.array_equal(n1[empty], ((1.0 - lr) * cs.nat1)[empty]) and np.array_equal(n2[empty], ((1.0 - lr) * o2)[empty]), tag
    if not packed:
        assert np.array_equal(n2[own], np.swapaxes(n2[own], -1, -2)), "the dense site is not symmetric to the bit"


@pytest.mark.parametrize("d", DIMS)
def test_site_update(amd, d):
    """mfgm_sparse_site_update and mfgm_sparse_site_update_q at every d, M + 1 in {2, 3, 31, 32, 33, 64, 65, 70} and lr in {0.7, 1}."""
    test = "test_site_update"
    for M1, ends in SITE_CASES:
        cs = case(d, M1, ends)
        D = Dev(amd, cs)
        E = Dev(amd, cs, empty=True)
        runs = {}
        for packed in (False, True):
            for lr in np_sparse.LRS:
                tag = f"d={d} M+1={M1}{'' if ends else ' empty ends'} lr={lr} {'packed' if packed else 'dense'}"
                got = runs[(packed, lr)] = D.update(lr, packed)
                check_sites(test, tag, D, got, d, M1, ends, lr, packed)
                again = D.update(lr, packed)
                assert np.array_equal(got[1], again[1]) and np.array_equal(got[2], again[2]), "two launches differ"
            # lr = 1 leaves no trace of the old sites (`got` is the lr = 1 run)
            other = D.update(1.0, packed, nat1=3.0 * cs.nat1 + 1.0, nat2=-2.0 * cs.nat2)
            assert np.array_equal(got[1], other[1]) and np.array_equal(got[2], other[2]), "lr = 1 kept something of the old sites"
            # N = 0 with null w, c, g1, g2: every site decays
            rc, n1, n2 = E.update(0.7, packed)
            o2 = np_sparse.pack(np.asarray(cs.nat2), d) if packed else cs.nat2
            assert rc == 0 and np.array_equal(n1, (1.0 - 0.7) * cs.nat1) and np.array_equal(n2, (1.0 - 0.7) * o2)
        # the dense kernel takes the roundings of the packed one: the packed sites, unpacked, are the dense sites bit for bit
        for lr in np_sparse.LRS:
            dn, pk = runs[(False, lr)], runs[(True, lr)]
            assert np.array_equal(dn[1], pk[1]) and np.array_equal(dn[2], np_sparse.unpack(pk[2], d)), "dense and packed sites differ"


@pytest.mark.parametrize("d", SHARD_DIMS)
def test_shards(amd, d):
    """One chain shared between processes: (0, k), (k, M + 1), (k, k + 1) and a middle range of 37 intervals (no multiple of 4, 8 or
    32), the per-point arrays holding the owned points only."""
    test = "test_shards"
    M1, ends, k = 70, True, 11
    cs = case(d, M1, ends)
    whole = Dev(amd, cs)
    plan = plan_of(amd, cs.M, d) if d > 8 else None
    full = whole.predict(plan)
    full_sites = {(lr, packed): whole.update(lr, packed) for lr in np_sparse.LRS for packed in (False, True)}
    sums = {}
    for own in ((0, k), (k, M1), (k, k + 1), (9, 46)):
        D = Dev(amd, cs, own=own)
        tag = f"d={d} shard {own}"
        got = D.predict(plan)
        check_predict(test, tag, D, got, d, M1, ends, plan)
        assert np.array_equal(got[1], full[1][D.pts]) and np.array_equal(got[2], full[2][D.pts]), "a shard's predictions differ from the whole"
        sums[own] = (got[3], got[4])
        for (lr, packed), fs in full_sites.items():
            gs = D.update(lr, packed)
            check_sites(test, f"{tag} lr={lr} {'packed' if packed else 'dense'}", D, gs, d, M1, ends, lr, packed)
            sl = slice(*own)
            assert np.array_equal(gs[1][sl], fs[1][sl]) and np.array_equal(gs[2][sl], fs[2][sl]), "a shard's sites differ from the whole"
    if plan is not None:
        kl = np_sparse.kl_terms(cs)
        for j, (name, a) in enumerate((("trace", kl.atrace), ("maha", kl.amaha))):
            held(test, f"d={d} shard sums add up, {name}", sums[(0, k)][j] + sums[(k, M1)][j], full[3 + j], a, 2 * d * d * kl.nodes)
        plan.check_info()


def run_cond(amd, cs, q):
    from vidp_amd import _lib
    from vidp_amd.packed import _ptr as p, _stream
    import torch
    d = cs.d
    b = [dev(q.idx, np.int32), dev(q.P), dev(q.T), dev(cs.pm), dev(cs.P0), dev(cs.mu), dev(cs.Sig), dev(cs.Sub)]
    mean, cov = sent(q.N + PAD, d), sent(q.N + PAD, d, d)
    rc = _lib.load().mfgm_cond_predict(cs.M, d, q.N, *(p(x) for x in b), p(mean), p(cov), _stream())
    torch.cuda.synchronize()
    mean, cov = host(mean), host(cov)
    assert np.all(mean[q.N:] == SENT) and np.all(cov[q.N:] == SENT), "written behind the last query point"
    return rc, mean[:q.N], cov[:q.N]


@pytest.mark.parametrize("d", DIMS)
def test_cond_predict(amd, d):
    """mfgm_cond_predict at every d: one query point, and forty with idx unsorted, repeated and holding 0, 1, M - 1 and M; M = 69, 1 and
    2; out_cov compared in full.  d = 32 takes 66 048 B of dynamic LDS, above the 65 536 other entry points of the library refuse: the
    launch has to succeed and be right (finding in the module docstring)."""
    test = "test_cond_predict"
    for M1 in (70, 2, 3):
        cs = case(d, M1, True)
        for N in (1, 40):
            q = np_sparse.make_queries(cs, N)
            if N == 40:
                assert {0, 1, cs.M - 1, cs.M} <= set(q.idx.tolist()) and len(set(q.idx.tolist())) < N
            want = np_sparse.cond_predict(cs, q)
            rc, mean, cov = run_cond(amd, cs, q)
            assert rc == 0, (d, M1, N, rc)
            held(test, f"d={d} M+1={M1} N={N} mean", mean, want[0], want[2], 2 * d)
            held(test, f"d={d} M+1={M1} N={N} cov", cov, want[1], want[3], 4 * d * d + 1)
            again = run_cond(amd, cs, q)
            assert np.array_equal(mean, again[1]) and np.array_equal(cov, again[2])
        none = np_sparse.SimpleNamespace(N=0, idx=np.zeros(1, np.int32), P=np.zeros((1, d, 2 * d)), T=np.zeros((1, d, d)))
        assert run_cond(amd, cs, none)[0] == 0          # N = 0: returns 0, and (checked inside) writes nothing


@pytest.mark.parametrize("d", DIMS)
def test_theta(amd, d):
    """mfgm_sparse_theta at every d with T in {1, 2, 37}, plin given and NULL; the last node's sub block is exactly zero."""
    from vidp_amd import _lib
    from vidp_amd.packed import _ptr as p, _stream
    import torch
    test = "test_theta"
    cs = case(d, 70, True)
    for T in (1, 2, 37):
        for with_plin in (True, False):
            want = np_sparse.theta(cs, T, with_plin)
            b = [dev(cs.nat1[:T + 1]), dev(cs.nat2[:T + 1]), dev(cs.plin[:T]) if with_plin else None, dev(cs.pdiag[:T]), dev(cs.psub[:T])]
            out = [sent(T + 1, d), sent(T + 1, d, d), sent(T + 1, d, d)]
            rc = _lib.load().mfgm_sparse_theta(T, d, *(p(x) for x in b), *(p(x) for x in out), _stream())
            torch.cuda.synchronize()
            assert rc == 0
            o = [host(x) for x in out]
            for k, name in enumerate(("lin", "diag", "sub")):
                assert np.all(o[k][T] == SENT), "written behind the last node"
                held(test, f"d={d} T={T} plin={'given' if with_plin else 'NULL'} {name}", o[k][:T], want[k], want[3 + k], 3)
            assert np.all(o[2][T - 1] == 0.0)


def test_argument_checks(amd):
    """What the entry points refuse before launching anything: d = 33, M = 0, m_lo >= m_hi, m_hi > M + 1 and null outputs return
    non-zero and leave every output at the sentinel."""
    from vidp_amd import _lib
    from vidp_amd.packed import _ptr as p, _stream
    import torch
    lib = _lib.load()
    d, M1 = 12, 33
    cs = case(d, M1, True)
    plan = plan_of(amd, cs.M, d)

    def bad(**kw):
        D = Dev(amd, cs)
        for k, v in kw.items():
            setattr(D.sd, k, v)
        D.m_lo, D.m_hi = 0, 0          # nothing is owned as far as the sentinel check of update() goes: every site must stay
        return D

    for kw in (dict(d=33), dict(M=0), dict(m_lo=5, m_hi=5), dict(m_lo=6, m_hi=5), dict(m_lo=0, m_hi=M1 + 1), dict(m_lo=-1, m_hi=4), dict(d=0)):
        D = bad(**kw)
        for pl in (None, plan):
            rc, fmu, fvar, tr, mh = D.predict(pl)
            assert rc != 0 and np.all(fmu == SENT) and np.all(fvar == SENT) and tr == SENT and mh == SENT, kw
        for packed in (False, True):
            assert D.update(0.7, packed)[0] != 0, kw
    # null outputs
    D = Dev(amd, cs)
    k = D.keep
    out, kt = sent(2, D.N), sent(2)
    mu, Sig, Sub = p(k["mu"]), p(k["Sig"]), p(k["Sub"])
    for fm, fv in ((None, out[1]), (out[0], None)):
        assert lib.mfgm_sparse_predict(ctypes.byref(D.sd), mu, Sig, Sub, p(fm), p(fv), _stream()) != 0
        assert lib.mfgm_sparse_predict_kl(ctypes.byref(D.sd), mu, Sig, Sub, p(fm), p(fv), plan.h, p(k["Pd"]), p(k["Ps"]), cs.aD, cs.aS,
                                          p(k["mup"]), p(kt[0:1]), p(kt[1:2]), p(plan.ws), _stream()) != 0
    for t, m in ((None, kt[1:2]), (kt[0:1], None)):
        assert lib.mfgm_sparse_predict_kl(ctypes.byref(D.sd), mu, Sig, Sub, p(out[0]), p(out[1]), plan.h, p(k["Pd"]), p(k["Ps"]), cs.aD, cs.aS,
                                          p(k["mup"]), p(t), p(m), p(plan.ws), _stream()) != 0
    n1, n2, n2q = sent(M1, 2 * d), sent(M1, 2 * d, 2 * d), sent(M1, d * (d + 1) + d * d)
    for a, b in ((None, n2), (n1, None)):
        assert lib.mfgm_sparse_site_update(ctypes.byref(D.sd), p(k["g1"]), p(k["g2"]), 0.7, p(a), p(b), _stream()) != 0
    for a, b in ((None, n2q), (n1, None)):
        assert lib.mfgm_sparse_site_update_q(ctypes.byref(D.sd), p(k["g1"]), p(k["g2"]), 0.7, p(a), p(b), _stream()) != 0
    q = np_sparse.make_queries(cs, 4)
    b = [dev(q.idx, np.int32), dev(q.P), dev(q.T), dev(cs.pm), dev(cs.P0), dev(cs.mu), dev(cs.Sig), dev(cs.Sub)]
    mean, cov = sent(4, d), sent(4, d, d)
    for args in ((cs.M, 33, 4), (0, d, 4), (cs.M, d, -1)):
        assert lib.mfgm_cond_predict(*args, *(p(x) for x in b), p(mean), p(cov), _stream()) != 0
    for a, c in ((None, cov), (mean, None)):
        assert lib.mfgm_cond_predict(cs.M, d, 4, *(p(x) for x in b), p(a), p(c), _stream()) != 0
    th = [sent(3, d), sent(3, d, d), sent(3, d, d)]
    tb = [dev(cs.nat1[:4]), dev(cs.nat2[:4]), dev(cs.plin[:3]), dev(cs.pdiag[:3]), dev(cs.psub[:3])]
    for T, dd in ((0, d), (3, 33), (3, 0)):
        assert lib.mfgm_sparse_theta(T, dd, *(p(x) for x in tb), *(p(x) for x in th), _stream()) != 0
    for j in range(3):
        o = list(th)
        o[j] = None
        assert lib.mfgm_sparse_theta(3, d, *(p(x) for x in tb), *(p(x) for x in o), _stream()) != 0
    torch.cuda.synchronize()
    for x in (out, kt, n1, n2, n2q, mean, cov, *th):
        assert bool((x == SENT).all())


def test_predict_fallback_route_in_a_child(amd, tmp_path):
    """k_sparse_predict<D2P> at even d: MFGM_SPARSE_PREDICT_V=0 is read once per process, so tests/mp_sparse_predict.py runs every even
    d in one fresh child with it set and leaves its outputs in a file; they are held to the same reference and bound here.  That the
    child took another route than this process shows in the bits: the two routes sum in another order."""
    test = "test_predict_fallback_route_in_a_child"
    path = str(tmp_path / "fallback.npz")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MFGM_SPARSE_PREDICT_V="0")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "mp_sparse_predict.py"), path], env=env, timeout=300, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.load(path)
    differs = 0
    for d in range(2, 33, 2):
        for M1, ends in PREDICT_CASES:
            cs = case(d, M1, ends)
            D = Dev(amd, cs)
            key = f"{d}_{M1}_{int(ends)}"
            for kl in (False, True) if d > 8 else (False,):
                plan = plan_of(amd, cs.M, d) if kl else None
                tr, mh = got[f"kl_{key}"] if kl else (SENT, SENT)
                child = (0, got[f"fmu_{key}_{int(kl)}"], got[f"fvar_{key}_{int(kl)}"], tr, mh)
                check_predict(test, f"d={d} M+1={M1}{'' if ends else ' empty ends'}{' kl' if kl else ''} (child)", D, child, d, M1, ends, plan)
                here = D.predict(plan)
                differs += int(not np.array_equal(here[2], child[2]))
    assert differs > 20, "the child's outputs are those of the coalesced route bit for bit: the fallback was not taken"
