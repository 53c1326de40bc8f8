"""
GPU tests of the fused Kalman filter with sites -- the four entry points mfgm_kf_sites_loglik / _elbo / _predict / _predict_factored
(csrc/mfgm_api_sweeps.hip), the local kernels k_kf_assemble<D, O> and k_kf_project<D, O> (csrc/mfgm_kf.h), the two-stage reduction
k_kf_elbo_stage1 / k_kf_elbo_stage2 and both routes of launch_sum_partials -- through the C ABI, against the 80-bit host reference
tests/np_kf.py, at every (d, o) with d = 1 ... 8 and o = 1, 2, on inputs in which no mapping mistake cancels (np_kf.make_case).
Packed outputs are pre-filled with a sentinel; natural-layout outputs have a sentinel pad behind them that must survive.

Cases (np_kf.CASES; B, T, R0), each at all 16 (d, o):
  (3, 37, 4)  twice: shared sites, non-zero mean, Hmu and plin given | per-chain sites, zero mean, Hmu and plin NULL.  10 segments,
              the last one holds one node.  (Two levels: ten level-1 nodes are swept by one lane.  Three levels come with the next.)
  (3, 37, 2)  19 segments, the last one holds one node; three levels; shared sites with a zero mean
  (70, 9, 2)  350 lanes: b changes inside a 64-lane block, the last block is padded
  (2, 1, 0)   T = 1, Ps NULL          (2, 2, 0)   single-level plan          (2, 8, 8)   T = R0: single level, one full segment
              (T = 1: the rounding of Sig, x, Fmu and Fvar is checked at d = 2 ... 8, on random inputs with cond_2 ~ 1e2; at d = 1
              the inputs are exact -- "The scalar case" below -- and only the mapping is checked there.)
  (1, 16385, 2) at (d, o) = (2, 1) and (1, 2) only: P = 8193 >= 8192 with B == 1, k_sum_partials_split in loglik, elbo's stage 1 at
              slice 129; cond_2 there is the largest one over dense windows of 64 nodes (every 32 nodes), not that of the whole.

Tolerance rule.  EPS = 2^-52; every check prints err / bound and asserts <= 1; no entry is skipped, entries with a zero bound are
compared exactly.
  Local (D, r, t1, ldR, and Fmu / Fvar against the 80-bit projection of the device's own x and Sig): sums of products of the inputs,
    |got - want| <= 4 n EPS sum|terms| (the rule of tests/test_gpu_sparse.py), n = o^2 + 1 (D), o (o + 1) + 1 (r), d (Fmu), d^2
    (Fvar), T o (t1, ldR); sum|terms| from the reference, carrying (|ad| + |bc|) / |det| of the 2 x 2 solve for o = 2, and
    1 + |log det| per term of ldR.
  Sweep (through the factorisation and the selected inverse): the bound tests/test_gpu_accuracy.py holds for the Cholesky form.
    Sig, x, Fmu, Fvar: max|got - want| <= 0.5 EPS cond_2 max|want|, per output and chain.  logdet, quad, ll, total:
    |got - want| <= (0.5 cond_2 + 4 n) EPS sum|terms|, n the number of summed terms.  cond_2: of the dense posterior precision.
  np_kf.make_case spreads the coordinates of the prior over a factor 12, so that cond_2 is 1e2 ... 1e4 wherever the problem has more
  than one unknown.

The scalar case.  At d = 1, T = 1 the system is one number: cond_2 = 1, and the sweep bound of the array outputs is half an ulp of
the largest entry, which no fp64 route through a square root and two divisions holds on general inputs (the float64 twin of the
reference missed it by factors 1.6 ... 2.7 on random ones, and so did the kernels).  The bound is kept as stated, and
np_kf.scalar_system gives that case inputs on which fp64 rounds nothing on the way to Sig, x, Fmu and Fvar: short binary fractions,
with the prior chosen so that D = Pd + h R^{-1} h is 4 or 16 exactly.  A mapping mistake still shows in full; t1, ldR, logdet and ll
of that case are rounded as everywhere.

What the dispatch can launch, and the test that launches it:
  k_kf_assemble<D, O>, D = 1 ... 8, O = 1, 2 (16)   mode 0: test_loglik, test_elbo; mode 1: test_predict -- all 16, every case
  k_kf_project<D, O>, the same 16                   test_predict, test_predict_factored
  mfgm_kf_sites_loglik                              test_loglik          mfgm_kf_sites_elbo               test_elbo
  mfgm_kf_sites_predict                             test_predict         mfgm_kf_sites_predict_factored   test_predict_factored
  launch_sum_partials, one k_sum_partials           test_loglik, every case but the long one (P < 8192 or B > 1)
  launch_sum_partials, k_sum_partials_split         test_loglik[d2-o1-long], [d1-o2-long]
  k_kf_elbo_stage1 / stage2                         test_elbo (slice 1 at P <= 64; 129 in the long case), test_python_route
  Hmu and plin given | NULL                         cases 0, 3 ... 6 | cases 1, 2
  site_batch 1 | B                                  cases 0, 2 (B = 3) | the others; test_python_route both

Largest err / bound measured on an MI355X per test over every (d, o) and case (a test passes when <= 1), next to the float64 twin's
over the same cases (tests/test_host_kf.py):
  test_loglik              D 0.128 (d = 8, o = 1, B = 70), r 0.074, t1 0.159, ldR 0.066, logdet 0.194 (d = 1, T = 1), quad 0.057
  test_elbo                t1 0.159, ldR 0.066, logdet 0.194, quad 0.057, ll 0.016, total 0.005; terms against loglik's outputs below
                           0.00005 in every case, the long one included; every NULL combination and repeat bit-identical
  test_predict             r 0.042, Sig 0.058, x 0.087, Fmu 0.324 (d = 6, o = 1, T = 1), Fvar 0.063, Fmu / Fvar of own x, Sig 0.125
  test_predict_factored    bit-identical to predict in every case; after elbo: Sig 0.036, x 0.033, Fmu 0.026, Fvar 0.032
  test_python_route        fused, unfused and their difference 0.001 of the bound of total
  float64 twin             D 0.128, r 0.089 / 0.066 (mode 0 / 1), t1 0.159, ldR 0.066, logdet 0.034, quad 0.029, ll 0.016, total 0.004,
                           Sig 0.058, x 0.076, Fmu 0.292 (d = 7, o = 1, T = 1), Fvar 0.063, Fmu / Fvar of own x, Sig 0.125

What these tests found.  No error in the kernels: all 16 instantiations of both local kernels, both summation routes, both stages of
the ELBO reduction and every NULL combination hold their bounds and their bit identities.  One error in kalman_filter.py, on the
route the fused one is compared with: with VIDP_FUSED_KF=0 (or any model the fused route declines) and B > 1 chains,
KalmanFilterWithSites.log_likelihood() raised on sites given per chain as (B T, o) -- _rinv_full and _obs tried to expand the flat
[B T, ...] tensors to [B, T, ...] -- and _log_det_observation_precision would have added the sum over all chains to every chain.
Fixed there: flat per-chain sites are reshaped to [B, T, ...] and their log-determinants summed per chain; test_python_route holds
the fused and the unfused totals to each other and to the 80-bit total.  The array sweep bound cannot be held on general inputs by a
chain of one node with d = 1 (the scalar case above).

Checked once with three deliberately wrong scratch builds of the library (not committed; arithmetic only, no address, index bound or
launch shape changed), each against this file without the long cases and against the older tests that reach the path
(test_kalman_filter_sites_golden, test_kalman_filter_sites_fused_output_dim_2, test_cvi_gaussian_process).
(a) nat2 is symmetric to the bit, so R^{-1}[a][c] swapped for R^{-1}[c][a] in k_kf_assemble changes nothing; instead the hm[c]
subtraction dropped for c = 1: test_loglik and test_elbo fail at all eight d with o = 2 in the five cases that have a prior mean (80
ids), test_python_route at all five d with o = 2; o = 1, the zero-mean cases and (r of mode 1 does not read hm) test_predict pass.
Of the older tests test_kalman_filter_sites_fused_output_dim_2 sees it (both ids: d = 3, o = 2, a prior mean); the other two do not.
(b) the chain of a site: reading a shared site array at chain b would read past its end, so the mutation went the other way, chain 0
always, which stays inside every array: test_loglik, test_elbo and test_predict fail at all 16 (d, o) in the five cases with
per-chain sites, test_predict_factored in the zero-mean one of them, test_python_route at all ten (d, o), and the good call of
test_rejections_and_not_pd; the shared-site cases pass.  Of the older tests only test_kalman_filter_sites_fused_output_dim_2[b3]
sees it.  (c) + s[3] for + 0.5 s[3] in k_kf_elbo_stage2: test_elbo fails at all 16 (d, o) in all seven cases (ll and total; terms
still hold), test_python_route at all ten, test_rejections_and_not_pd; all three older tests see it (six ids).
"""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from tests import np_kf

pytestmark = pytest.mark.gpu

SENT = -7.0e77            # sentinel the outputs are pre-filled with
PAD = 8                   # sentinel entries behind every natural-layout output
WORST = {}


def _id(d, o, case):
    B, T, R0, shared, zm = case
    return f"d{d}-o{o}-" + ("long" if T > 10000 else f"B{B}T{T}R{R0}{'s' if shared else ''}{'z' if zm else ''}")


PARAMS = [pytest.param(d, o, case, id=_id(d, o, case)) for d, o in np_kf.DIMS for case in np_kf.cases_of(d, o)]


@pytest.fixture(scope="module")
def amd():
    import torch
    import vidp_amd
    assert torch.cuda.is_available()
    vidp_amd._lib.load()
    yield vidp_amd
    _PLANS.clear()            # the plans of this module (two of them T = 16385) go with it


def dev(x, dtype=np.float64):
    import torch
    return torch.from_numpy(np.array(x, dtype=dtype, order="C")).cuda()          # a copy: the cases are read-only


def host(x):
    return x.detach().cpu().numpy()


def sent(n):
    import torch
    return torch.full((n,), SENT, dtype=torch.float64, device="cuda")


def held(test, tag, ratios):
    """Print and assert a dict {output: err / bound} of the np_kf checks."""
    for name, r in ratios.items():
        w = WORST.setdefault(test, {})
        if name not in w or r > w[name][0]:
            w[name] = (r, tag)
        print(f"  {test} {tag} {name}: err / bound {r:.4f}  (largest so far in this test {w[name][0]:.4f}, {w[name][1]})")
    for name, r in ratios.items():
        assert r <= 1.0, (test, tag, name, r)


# ---- references, computed once and shared ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kcase(d, o, case):
    B, T, R0, shared, zm = case
    return np_kf.make_case(d, o, B, T, shared, zm)


@functools.lru_cache(maxsize=None)
def kref(d, o, case):
    return np_kf.reference(kcase(d, o, case))


_PLANS = {}


def plan_of(amd, B, T, d, R0):
    if (B, T, d, R0) not in _PLANS:
        _PLANS[(B, T, d, R0)] = amd.Plan(B, T, d, R0=R0)
    return _PLANS[(B, T, d, R0)]


# ---- device side ---------------------------------------------------------------------------------------------------------------------------
class Run:
    """The device arrays of a case and the four calls of the C ABI.  Every call takes fresh, sentinel-filled outputs, synchronises,
    checks the pads and returns host arrays (packed ones unpacked)."""

    def __init__(self, amd, cs, R0, nat2=None):
        import torch
        from vidp_amd import _lib
        from vidp_amd.packed import _ptr, _stream
        self.torch, self.p, self._stream, self.amd, self.cs = torch, _ptr, _stream, amd, cs
        self.lib = _lib.load()
        self.plan = pl = plan_of(amd, cs.B, cs.T, cs.d, R0)
        self.Pd = pl.pack(amd.SYM, dev(cs.Pd))
        self.Ps = pl.pack(amd.FULL, dev(cs.Ps)) if cs.T > 1 else None
        self.plin = pl.pack(amd.VEC, dev(cs.plin)) if cs.plin is not None else None
        self.n1, self.n2 = dev(cs.nat1), dev(cs.nat2 if nat2 is None else nat2)
        self.Hmu = dev(cs.Hmu) if cs.Hmu is not None else None
        self.slc = dev(cs.sumlogchol)
        self.sv = self.sites()
        self.n = cs.B * cs.T * cs.o

    def sites(self, o=None, site_batch=None, nat1=True, nat2=True):
        from vidp_amd import _lib
        cs = self.cs
        sv = _lib.KfSites()
        for i, v in enumerate(cs.H.reshape(-1).tolist()):
            sv.H[i] = v
        sv.o, sv.site_batch = (cs.o if o is None else o), (cs.Bs if site_batch is None else site_batch)
        sv.nat1, sv.nat2 = (self.n1.data_ptr() if nat1 else None), (self.n2.data_ptr() if nat2 else None)
        sv.Hmu = self.Hmu.data_ptr() if self.Hmu is not None else None
        return sv

    def packed(self, *kinds):
        return [self.plan.empty(k).fill_(SENT) for k in kinds]

    def unpack(self, kind, x):
        return host(self.plan.unpack(kind, x))

    def nat(self, x, n, shape=None):
        x = host(x)
        assert np.all(x[n:] == SENT), "written behind the end of a natural-layout output"
        return x[:n] if shape is None else x[:n].reshape(shape)

    def loglik(self):
        a, cs, p = self.amd, self.cs, self.p
        D, r, L, y = self.packed(a.SYM, a.VEC, a.TRI, a.VEC)
        s = [sent(cs.B + PAD) for _ in range(4)]
        rc = self.lib.mfgm_kf_sites_loglik(self.plan.h, ctypes.byref(self.sv), p(self.Pd), p(self.Ps), p(D), p(r), p(L), p(y), *(p(x) for x in s),
                                           p(self.plan.ws), p(self.plan.info), self._stream())
        self.torch.cuda.synchronize()
        assert rc == 0, rc
        self.plan.check_info()
        t1, ldR, logdet, quad = (self.nat(x, cs.B) for x in s)
        return SimpleNamespace(D=self.unpack(a.SYM, D), r=self.unpack(a.VEC, r), t1=t1, ldR=ldR, logdet=logdet, quad=quad)

    def elbo(self, terms=True, ll=True, total=True, check=True):
        """(rc, terms [4, B], ll [B], total, L, y): the outputs asked for; the others NULL, their buffers still the sentinel."""
        a, cs, p = self.amd, self.cs, self.p
        D, r, L, y = self.packed(a.SYM, a.VEC, a.TRI, a.VEC)
        tb, lb, ob = sent(4 * cs.B + PAD), sent(cs.B + PAD), sent(1 + PAD)
        rc = self.lib.mfgm_kf_sites_elbo(self.plan.h, ctypes.byref(self.sv), p(self.Pd), p(self.Ps), p(D), p(r), p(L), p(y), p(self.slc),
                                         float(cs.cst), p(tb if terms else None), p(lb if ll else None), p(ob if total else None),
                                         p(self.plan.ws), p(self.plan.info), self._stream())
        self.torch.cuda.synchronize()
        if check and rc == 0:
            self.plan.check_info()
        return rc, self.nat(tb, 4 * cs.B, (4, cs.B)), self.nat(lb, cs.B), self.nat(ob, 1)[0], L, y

    def predict(self):
        a, cs, p = self.amd, self.cs, self.p
        D, r, L, y, Sig, x = self.packed(a.SYM, a.VEC, a.TRI, a.VEC, a.SYM, a.VEC)
        Fmu, Fvar = sent(self.n + PAD), sent(self.n + PAD)
        rc = self.lib.mfgm_kf_sites_predict(self.plan.h, ctypes.byref(self.sv), p(self.Pd), p(self.Ps), p(self.plin), p(D), p(r), p(L), p(y),
                                            p(Sig), p(x), p(Fmu), p(Fvar), p(self.plan.ws), p(self.plan.info), self._stream())
        self.torch.cuda.synchronize()
        assert rc == 0, rc
        self.plan.check_info()
        shp = (cs.B, cs.T, cs.o)
        return SimpleNamespace(r=self.unpack(a.VEC, r), Sig=self.unpack(a.SYM, Sig), x=self.unpack(a.VEC, x), Fmu=self.nat(Fmu, self.n, shp),
                               Fvar=self.nat(Fvar, self.n, shp), L=L, y=y, Sig_p=host(Sig), x_p=host(x))

    def predict_factored(self, L, y):
        a, cs, p = self.amd, self.cs, self.p
        Sig, x = self.packed(a.SYM, a.VEC)
        Fmu, Fvar = sent(self.n + PAD), sent(self.n + PAD)
        rc = self.lib.mfgm_kf_sites_predict_factored(self.plan.h, ctypes.byref(self.sv), p(self.Ps), p(L), p(y), p(Sig), p(x), p(Fmu), p(Fvar),
                                                     p(self.plan.ws), self._stream())
        self.torch.cuda.synchronize()
        assert rc == 0, rc
        shp = (cs.B, cs.T, cs.o)
        return SimpleNamespace(Sig=self.unpack(a.SYM, Sig), x=self.unpack(a.VEC, x), Fmu=self.nat(Fmu, self.n, shp),
                               Fvar=self.nat(Fvar, self.n, shp), Sig_p=host(Sig), x_p=host(x))


def check_plan(plan, case):
    """The partition is the one the case is there for."""
    B, T, R0, _, _ = case
    if (B, T, R0) in ((2, 1, 0), (2, 2, 0), (2, 8, 8)):
        assert plan.nlevels == 1
    if (B, T, R0) == (3, 37, 4):
        assert plan.P == 10 and plan.nlevels == 2
    if (B, T, R0) == (3, 37, 2):
        assert plan.P == 19 and plan.nlevels >= 3
    if (B, T, R0) == (70, 9, 2):
        assert plan.P == 5 and plan.Lpad == 384
    if T > 10000:
        assert B == 1 and plan.P == 8193


@pytest.mark.parametrize("d,o,case", PARAMS)
def test_loglik(amd, d, o, case):
    """mfgm_kf_sites_loglik: unpacked D and r against the mode-0 reference, t1 and ldR (local bound), logdet and quad (sweep bound); D
    symmetric to the bit."""
    test, tag = "test_loglik", _id(d, o, case)
    cs, ref = kcase(d, o, case), kref(d, o, case)
    R = Run(amd, cs, case[2])
    check_plan(R.plan, case)
    g = R.loglik()
    held(test, tag, np_kf.local_checks(cs, ref, g.D, g.r, None, g.t1, g.ldR))
    held(test, tag, np_kf.sweep_scalar_checks(cs, ref, logdet=g.logdet, quad=g.quad))
    assert np.array_equal(g.D, np.swapaxes(g.D, -1, -2)), "D is not symmetric to the bit"


@pytest.mark.parametrize("d,o,case", PARAMS)
def test_elbo(amd, d, o, case):
    """mfgm_kf_sites_elbo: terms [4, B] = (t1, ldR, log|L|, |y|^2) against the reference and against loglik's outputs (another order of
    summation: within the same bounds of each other), ll[b] and total; every combination of NULL terms / ll / total leaves the others
    bit-identical and the NULL ones' buffers untouched; ll and total both NULL returns 1; two calls give the same bits."""
    test, tag = "test_elbo", _id(d, o, case)
    cs, ref = kcase(d, o, case), kref(d, o, case)
    R = Run(amd, cs, case[2])
    rc, terms, ll, total, _, _ = R.elbo()
    assert rc == 0
    held(test, tag, np_kf.local_checks(cs, ref, None, None, None, terms[0], terms[1]))
    held(test, tag, np_kf.sweep_scalar_checks(cs, ref, logdet=terms[2], quad=terms[3], ll=ll, total=total))
    g = R.loglik()
    held(test, tag, {"t1 against loglik's": np_kf.ratio_local(terms[0], g.t1, ref.m0.at1, cs.T * o),
                     "ldR against loglik's": np_kf.ratio_local(terms[1], g.ldR, ref.m0.aldR, cs.T * o),
                     "logdet against loglik's": np_kf.ratio_scalar(terms[2], g.logdet, ref.alogdet, cs.T * d, cs.cond),
                     "quad against loglik's": np_kf.ratio_scalar(terms[3], g.quad, ref.quad, cs.T * d, cs.cond)})
    for wt in (True, False):
        for wl in (True, False):
            for wo in (True, False):
                rc2, t2, l2, o2, _, _ = R.elbo(wt, wl, wo)
                if not wl and not wo:
                    assert rc2 == 1 and np.all(t2 == SENT) and np.all(l2 == SENT) and o2 == SENT
                    continue
                assert rc2 == 0
                assert np.array_equal(t2, terms) if wt else np.all(t2 == SENT)
                assert np.array_equal(l2, ll) if wl else np.all(l2 == SENT)
                assert o2 == total if wo else o2 == SENT


@pytest.mark.parametrize("d,o,case", PARAMS)
def test_predict(amd, d, o, case):
    """mfgm_kf_sites_predict: unpacked r against the mode-1 reference; Sig, x, Fmu, Fvar (sweep bound); Fmu and Fvar against the 80-bit
    projection of the device's own x and Sig (local bound)."""
    test, tag = "test_predict", _id(d, o, case)
    cs, ref = kcase(d, o, case), kref(d, o, case)
    R = Run(amd, cs, case[2])
    g = R.predict()
    held(test, tag, np_kf.local_checks(cs, ref, None, None, g.r, None, None))
    held(test, tag, np_kf.project_checks(cs, g.Fmu, g.Fvar, g.x, g.Sig))
    assert np.array_equal(g.Sig, np.swapaxes(g.Sig, -1, -2))
    held(test, tag, np_kf.sweep_array_checks(cs, ref, g.Sig, g.x, g.Fmu, g.Fvar))


@pytest.mark.parametrize("d,o,case", PARAMS)
def test_predict_factored(amd, d, o, case):
    """mfgm_kf_sites_predict_factored on the (L, y) predict left, into fresh buffers: the same kernels on the same inputs, bit-identical
    Sig, x (packed arrays whole), Fmu, Fvar.  On the zero-mean cases also after elbo -- the reuse factored_for (kalman_filter.py)
    relies on: the sweep bound against the reference."""
    test, tag = "test_predict_factored", _id(d, o, case)
    cs, ref = kcase(d, o, case), kref(d, o, case)
    R = Run(amd, cs, case[2])
    g = R.predict()
    f = R.predict_factored(g.L, g.y)
    for name in ("Sig_p", "x_p", "Fmu", "Fvar"):
        assert np.array_equal(getattr(f, name), getattr(g, name)), name
    if cs.Hmu is None:
        rc, _, _, _, L, y = R.elbo()
        assert rc == 0
        f = R.predict_factored(L, y)
        held(test, tag, np_kf.project_checks(cs, f.Fmu, f.Fvar, f.x, f.Sig))
        held(test, tag, np_kf.sweep_array_checks(cs, ref, f.Sig, f.x, f.Fmu, f.Fvar))


def test_rejections_and_not_pd(amd):
    """What the entry points refuse (return 1, nothing written): o in {0, 3}, site_batch not in {1, B}, a wide plan (d = 9), each
    required pointer NULL in turn, Ps NULL with T > 1.  One site with nat2 > 0 large enough to make a pivot block indefinite: every
    ll[b] and total NaN, plan.check_info() raises ArithmeticError, and the next call on good inputs passes."""
    import torch
    from vidp_amd.packed import _ptr as p, _stream
    d, o, case = 3, 2, (3, 37, 4, False, True)
    cs, ref = kcase(d, o, case), kref(d, o, case)
    R = Run(amd, cs, case[2])
    a, lib, pl = amd, R.lib, R.plan
    D, r, L, y, Sig, x = R.packed(a.SYM, a.VEC, a.TRI, a.VEC, a.SYM, a.VEC)
    nat = [sent(4 * cs.B * cs.T * o + PAD) for _ in range(6)]
    sv = ctypes.byref(R.sv)
    calls = {
        "loglik": (lib.mfgm_kf_sites_loglik, [pl.h, sv, p(R.Pd), p(R.Ps), p(D), p(r), p(L), p(y), p(nat[0]), p(nat[1]), p(nat[2]), p(nat[3]),
                                              p(pl.ws), p(pl.info), _stream()], (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13)),
        "elbo": (lib.mfgm_kf_sites_elbo, [pl.h, sv, p(R.Pd), p(R.Ps), p(D), p(r), p(L), p(y), p(R.slc), float(cs.cst), p(nat[0]), p(nat[1]),
                                          p(nat[2]), p(pl.ws), p(pl.info), _stream()], (0, 1, 2, 3, 4, 5, 6, 7, 8, 13, 14)),
        "predict": (lib.mfgm_kf_sites_predict, [pl.h, sv, p(R.Pd), p(R.Ps), None, p(D), p(r), p(L), p(y), p(Sig), p(x), p(nat[4]), p(nat[5]),
                                                p(pl.ws), p(pl.info), _stream()], (0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14)),
        "predict_factored": (lib.mfgm_kf_sites_predict_factored, [pl.h, sv, p(R.Ps), p(L), p(y), p(Sig), p(x), p(nat[4]), p(nat[5]), p(pl.ws),
                                                                  _stream()], (0, 1, 2, 3, 4, 5, 6, 7, 8, 9)),
    }
    wide = amd.Plan(cs.B, cs.T, 9, R0=case[2])
    for name, (fn, args, required) in calls.items():
        for i in required:                                   # each required pointer NULL in turn (Ps is required: T > 1)
            bad = list(args)
            bad[i] = None
            assert fn(*bad) == 1, (name, i)
        for kw in (dict(o=0), dict(o=3), dict(site_batch=0), dict(site_batch=2), dict(site_batch=cs.B + 1), dict(nat1=False), dict(nat2=False)):
            bad = list(args)
            svb = R.sites(**kw)
            bad[1] = ctypes.byref(svb)
            assert fn(*bad) == 1, (name, kw)
        bad = list(args)
        bad[0] = wide.h
        assert fn(*bad) == 1, (name, "wide plan")
    bad = list(calls["elbo"][1])
    bad[11] = bad[12] = None
    assert calls["elbo"][0](*bad) == 1
    torch.cuda.synchronize()
    for t in (D, r, L, y, Sig, x, *nat):
        assert bool((t == SENT).all()), "a refused call wrote something"
    # not positive definite: R^{-1} = -1e6 I at one site of chain 1 makes D_5 of that chain indefinite (the prior's diagonal is below 1e4)
    n2 = np.array(cs.nat2)
    n2[1, 5] = 5.0e5 * np.eye(o)
    assert np.abs(cs.Pd).max() < 1e4
    Rb = Run(amd, cs, case[2], nat2=n2)
    rc, terms, ll, total, _, _ = Rb.elbo(check=False)
    assert rc == 0 and np.all(np.isnan(ll)) and np.isnan(total)
    with pytest.raises(ArithmeticError):
        pl.check_info()
    rc, terms, ll, total, _, _ = R.elbo()
    assert rc == 0
    held("test_rejections_and_not_pd", "after a not-PD call", np_kf.sweep_scalar_checks(cs, ref, ll=ll, total=total))


@pytest.mark.parametrize("o", [1, 2])
@pytest.mark.parametrize("d", [1, 4, 5, 7, 8])
def test_python_route(amd, monkeypatch, d, o):
    """KalmanFilterWithSites.log_likelihood() through fused_sites_call (kalman_filter.py), with the sites given once as (T, o) (shared)
    and once as (B T, o): site_batch deduced, H mu_prior computed and cached, cst.  Equal to the unfused route (VIDP_FUSED_KF=0) and to
    the 80-bit total -- of the prior precision, prior mean and sum-log-chol the model itself holds on the device -- within the sweep
    bound of total."""
    from tests.helpers import random_ssm_params
    from vidp_amd.emission_model import EmissionModel
    from vidp_amd.kalman_filter import GaussianSitesNat, KalmanFilterWithSites
    from vidp_amd.state_space_model import StateSpaceModel
    test = "test_python_route"
    B, T = 3, 9
    rng = np.random.default_rng([5501, d, o])
    prm = random_ssm_params(rng, (B,), T, d)
    ssm = StateSpaceModel(*[dev(x) for x in prm])
    pl = ssm.plan
    pr = ssm._precision_packed()
    Pd, Ps = host(pl.unpack(amd.SYM, pr["diag"])), host(pl.unpack(amd.FULL, pr["sub"], T - 1))
    mu_p = host(pl.unpack(amd.VEC, ssm._posterior_packed()["s"]["x"]))
    H = np_kf.make_H(d, o)
    em = EmissionModel(dev(np.broadcast_to(H, (B, T, o, d)).copy()), constant_matrix=dev(H))
    for shared in (True, False):
        cs = np_kf.make_case(d, o, B, T, shared, False, prior=(Pd, Ps, mu_p, host(pr["sumlogchol"])))
        ref = np_kf.reference(cs)
        sites = GaussianSitesNat(dev(cs.nat1.reshape(-1, o)), dev(cs.nat2.reshape(-1, o, o)))
        kf = KalmanFilterWithSites(ssm, em, sites)
        monkeypatch.delenv("VIDP_FUSED_KF", raising=False)
        fused = float(kf.log_likelihood())
        pl.check_info()
        monkeypatch.setenv("VIDP_FUSED_KF", "0")
        plain = float(kf.log_likelihood())
        monkeypatch.delenv("VIDP_FUSED_KF", raising=False)
        tag = f"d{d}-o{o}-{'shared' if shared else 'per-chain'}"
        held(test, tag, {"fused total": np_kf.sweep_scalar_checks(cs, ref, total=fused)["total"],
                         "unfused total": np_kf.sweep_scalar_checks(cs, ref, total=plain)["total"],
                         "fused - unfused": np_kf.ratio_scalar(fused, plain, ref.atotal, ref.n_total, cs.cond.max())})
