"""
GPU tests of the VDP kernels (csrc/mfgm_vdp.h, launched from csrc/mfgm_api_vdp.hip) against the 80-bit host reference tests/np_vdp.py,
through the C ABI, at every state dimension d = 1 ... 8 -- hence on the three branches of vdp_impl (d <= 5: both side passes ride in
the sweeps of mfgm_packed_vdp_marginals_products, d = 6: the products ride and the offsets pass follows, d = 7, 8: both follow) -- in
every mode of the fused sweep, with and without clipping, on the dense jump array and on obs_count / dobs_const, and at the edges of
the observations (nodes 0, 1, 2, T-2, T-1, the ends of a segment, two observations on a node, a chain without any).  Inputs come
from np_vdp.make_case: per-dimension af, bf, q all distinct, A_t not symmetric, a dense R^-1, nothing negligibly small.  Packed inputs
hold NaN wherever no node owns an entry and in the rows T-1 of (Am, bm), which stand for no transition; outputs are pre-filled with a
sentinel.

Tolerance rule (that of tests/test_gpu_cq.py).  Per output err = max |got - want| / max |want| against the 80-bit reference; the
yardstick is the same figure for the fp64 twin (the reference's code in np.float64) on the same inputs; bound = max(8 x yardstick,
64 eps).  On these inputs the yardstick is 0 ... 8 eps (tests/test_host_vdp.py prints it), so the floor of 64 eps = 1.4e-14 is what
binds nearly everywhere.  Every check prints err, yardstick, err / yardstick and err / bound; a check passes when err / bound <= 1.
The stages after the forward pass take the 80-bit marginals (and multipliers) rounded to fp64 as inputs, on the GPU as in the
reference and the twin; mode 3 of the fused sweep runs on the marginals its own products call produced, which are within the same
bound of those.  No output of a partitioned sweep needed a larger multiple.

Kernel instantiations and the test that launches them (D = 1 ... 8 everywhere):
  k_vdp_to_ssm<D>, k_vdp_to_naturals<D>                               test_vdp_to_ssm_and_naturals
  k_vdp_marginals<D, 1>, k_vdp_marginals<D, 3>, k_vdp_marginals_scan  test_vdp_marginals (and the D >= 6 / 7 routes of test_vdp_fused_routes)
  k_vdp_esde<D, true>, k_vdp_esde<D, false>, k_sum_partials           test_vdp_esde
  k_vdp_lagrange_products<D>, k_vdp_lagrange<D, 1>, <D, 3>,
  k_vdp_lagrange_scan_wave<D>                                         test_vdp_lagrange
  k_vdp_update_param<D>                                               test_vdp_update_param
  k_vdp_lagrange<D, 4> (mfgm_packed_vdp_lagrange_update, _final)      test_vdp_fused_routes
  k_vdp_lagrange<D, 5> (mfgm_packed_vdp_lagrange_update0 modes 0-3)   test_vdp_fused_routes
  k_vdp_marginals<D, 1, 1>  D <= 6                                    test_vdp_fused_routes (products call; D <= 5 only without jump terms)
  k_vdp_marginals<D, 3, 2>  D <= 5                                    test_vdp_fused_routes (products call with jump terms)
  NOT launched by any test: k_vdp_marginals<D, 1, 1> at D = 7, 8 and k_vdp_marginals<D, 3, 2> at D = 6, 7, 8, which vdp_impl never
  launches either; the quadrature VDP kernels (mfgm_quad_vdp_lagrange) have their own suite; k_congruence_scan and the band kernels,
  which share k_vdp_marginals_scan, are held in tests/test_gpu_api.py.

Largest err / bound measured on an MI355X, over every d, shape, variant and output of a test (a test passes when <= 1):
  test_vdp_to_ssm_and_naturals   0.033  (nat diag: err 4.7e-16, yardstick 2.4e-16)
  test_vdp_marginals             0.036  (S: err 5.2e-16, yardstick 3.6e-16)
  test_vdp_esde                  0.055  (double well dE/dS: err 7.8e-16, yardstick 7.8e-16)
  test_vdp_lagrange              0.031  (psi, no observations, obs_count form: err 4.4e-16, yardstick 2.4e-16); the dense and the
                                 obs_count form agree bit for bit at every d, shape and variant
  test_vdp_update_param          0.037  (b, clip, lr = 1: err 5.3e-16, yardstick 5.3e-16)
  test_vdp_fused_routes          0.061  (lam(0) of mode 3 after the products call with the dense jump array, clip: err 8.7e-16,
                                 yardstick 6.6e-16); mfgm_packed_vdp_lagrange_update_final and mode 1 bit-identical to the full calls
Where the yardstick is at least 1 eps, err / yardstick was at most 2.6: the partitioned sweeps (up to 65 segment maps) are as
accurate as the sequential fp64 loop on these contractive recurrences.

What these tests found.  With prm.clip small enough to clip the jump block, k_vdp_lagrange and k_vdp_marginals<D, 3, 2> formed
d_obs_m = yR + 2 dobsS m from the CLIPPED block, where the reference clips d_obs_m and d_obs_S each on its own: lam was off by 0.6 %
... 35 % of its largest entry in the "clip" variant of test_vdp_lagrange and test_vdp_fused_routes at every d (psi was right).  At
the reference's CLIP_MAX = 5000 no block is ever clipped, which is why the model-level tests never saw it.  Fixed in csrc/mfgm_vdp.h.

Checked once with two deliberately wrong scratch builds of the library (not committed).  (a) drift_moments reading pr.af[0] / pr.bf[0]
instead of index i fails, at every d >= 2 (d = 1 passes), every case of test_vdp_esde and test_vdp_update_param, every case of
test_vdp_lagrange but those of the one-transition chain (whose loop reads nothing), every case of test_vdp_fused_routes and the
"full" cases of test_vdp_marginals (e_over_dt) -- and passes the 24 VDP tests of tests/test_gpu_api.py (-k "vdp or
variational_markov"), which only ever use one scalar af, bf: the gap was real.  (b) the off-diagonal entries of dcst zeroed in
k_vdp_lagrange fails the obs_count form of test_vdp_lagrange ("full" and "clip", the three shapes with a loop) at every d >= 2 after
the dense form has passed, the same cases of test_vdp_fused_routes, and test_vdp_model_nonisotropic; d = 1, "noobs" and the
one-transition chain pass.
"""
import ctypes
import functools

import numpy as np
import pytest

from tests import np_vdp
from tests.np_vdp import LD

pytestmark = pytest.mark.gpu

DIMS = list(range(1, 9))
FLOOR = 64 * np_vdp.EPS
SENT = -7.0e77            # sentinel the outputs are pre-filled with
SHAPE_IX = list(range(len(np_vdp.SHAPES)))
WORST = {}


@pytest.fixture(scope="module")
def amd():
    import torch
    import vidp_amd
    assert torch.cuda.is_available()
    vidp_amd._lib.load()
    return vidp_amd


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(x):
    return x.detach().cpu().numpy()


# ---- references, computed once per (d, shape, variant) and shared -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(d, si, variant, kind="dw"):
    """(case with its 80-bit reference case.ref, the fp64 twin's outputs)."""
    case = np_vdp.make_case(d, np_vdp.SHAPES[si], variant, kind=kind)
    twin = np_vdp.reference(case, np.float64)
    for x in vars(case).values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return case, twin


@functools.lru_cache(maxsize=None)
def lagrange_without(d, si, node):
    """80-bit multipliers of the "full" case with the observations of one node taken away."""
    case, _ = reference(d, si, "full")
    yR, dobsS = case.yR.copy(), case.dobsS.copy()
    yR[:, node], dobsS[:, node] = 0.0, 0.0
    r = case.ref
    return np_vdp.lagrange(r.m64, r.S64, case.A, case.b, case.prm, yR, dobsS)


def held(test, name, got, want, twin, scale=None):
    """The tolerance rule of the module docstring; prints err, yardstick and the two ratios.  A reference that is exactly zero (lambda of
    a chain of one transition) is compared exactly."""
    want = np.asarray(want)
    assert np.all(np.isfinite(np.asarray(got, dtype=np.float64))), name
    if scale is None and np.abs(want).max() == 0:
        assert np.all(np.asarray(got) == 0), name
        return
    err, yard = np_vdp.rel_err(got, want, scale), np_vdp.rel_err(twin, want, scale)
    bound = max(8.0 * yard, FLOOR)
    WORST[test] = max(WORST.get(test, 0.0), err / bound)
    print(f"  {test} {name}: err {err:.3e}  yardstick {yard:.3e}  err / yardstick {err / yard if yard > 0 else float('inf'):.2f}  "
          f"err / bound {err / bound:.3f}  (largest err / bound so far in this test {WORST[test]:.3f})")
    assert err <= bound, (name, err, yard)


# ---- device side ------------------------------------------------------------------------------------------------------------------------------
class Dev:
    """The plan of a case, its packed device inputs and the calls of the C ABI."""

    def __init__(self, amd, case):
        import torch
        from vidp_amd import _lib
        from vidp_amd.packed import _ptr, _stream
        self.torch, self._ptr, self._stream, self._libmod = torch, _ptr, _stream, _lib
        self.case = c = case
        B, T, R0, Rup = c.shape
        self.plan = amd.Plan(B, T, c.d, R0=R0, Rup=Rup)
        lv = c.levels[0]
        assert (self.plan.R, self.plan.P, self.plan.Lpad) == (lv[1], lv[2], lv[3])
        self.lib, self.h, self.lv = self.plan.lib, self.plan.h, lv
        self.d, self.B, self.T = c.d, B, T
        self.Am, self.bm = self.rows(c.A.reshape(B, T - 1, -1)), self.rows(c.b)
        self.q0_mu, self.q0_cov = dev(c.q0_mu), dev(np_vdp.tril_pack(c.q0_cov))
        self.p0inv, self.p0lin = dev(np_vdp.tril_pack(c.p0inv)), dev(c.p0lin)
        self.yR, self.dobsS = self.pack(c.yR), self.pack(np_vdp.tril_pack(c.dobsS))
        self.obs_count = self.pack_counts(c.obs_count)
        self.dobs_const = dev(np_vdp.tril_pack(c.dobs_const))
        self.nseg = self.lib.mfgm_vdp_workspace_doubles(self.h)
        if hasattr(c.ref, "m64"):
            self.m, self.S = self.pack(c.ref.m64), self.pack(np_vdp.tril_pack(c.ref.S64))

    # layouts
    def pack(self, arr, fill=np.nan):
        """[B, T, E] -> packed device array; entries no node owns hold `fill`."""
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        return dev(np_vdp.pack_nodes(arr, self.lv, np.full(arr.shape[-1], fill)))

    def rows(self, arr):
        """[B, T-1, E] of the transitions -> packed, the row T-1 NaN."""
        arr = np.asarray(arr, dtype=np.float64)
        return self.pack(np.concatenate([arr, np.full((self.B, 1, arr.shape[-1]), np.nan)], axis=1))

    def pack_counts(self, counts):
        """obs_count in the packed order of include/mfgm.h:765-768, one int per node; entries no node owns hold 7."""
        return dev(np_vdp.pack_nodes(np.ascontiguousarray(counts[..., None], dtype=np.int32), self.lv, np.array([7], dtype=np.int32)))

    def out(self, E):
        return self.torch.full((self.lv[3] * self.lv[1] * E,), SENT, dtype=self.torch.float64, device="cuda")

    def flat(self, *shape):
        return self.torch.full(shape, SENT, dtype=self.torch.float64, device="cuda")

    def seg(self):
        return self.flat(max(self.nseg, 1))

    def unpack(self, t, E, rows=None):
        """(natural [B, rows, E], raw host copy): every entry no node owns, and every row >= rows, must still hold the sentinel."""
        raw = host(t)
        assert raw.size == self.lv[3] * self.lv[1] * E
        nat, own = np_vdp.unpack_nodes(raw, self.B, self.T, E, self.lv)
        assert np.all(raw[~own] == SENT), "an entry no node owns was written"
        rows = self.T if rows is None else rows
        assert np.all(nat[:, rows:] == SENT), "a row beyond the last one was written"
        assert not np.any(nat[:, :rows] == SENT), "an entry was not written"
        return nat[:, :rows], raw

    # parameters
    def prm(self, p=None, lr=0.0):
        p = self.case.prm if p is None else p
        s = self._libmod.VdpParams()
        d = self.d
        for i in range(d):
            s.af[i], s.bf[i], s.q[i], s.mu0[i] = p.af[i], p.bf[i], p.q[i], p.mu0[i]
        for k, v in enumerate(np_vdp.tril_pack(np.asarray(p.chol0))):
            s.chol0[k] = v
        s.dt, s.lr, s.clip = p.dt, float(lr), p.clip
        return s

    def call(self, name, *args):
        """An entry point of the C ABI on this plan: tensors and None become pointers, the parameter block goes by reference, an int (the
        mode of mfgm_packed_vdp_lagrange_update0) stays; the stream is appended."""
        conv = [ctypes.byref(a) if isinstance(a, ctypes.Structure) else a if isinstance(a, int) else self._ptr(a) for a in args]
        rc = getattr(self.lib, name)(self.h, *conv, self._stream())
        assert rc == 0, (name, rc)
        self.torch.cuda.synchronize()

    def jumps(self, form, yR=None, dobsS=None, counts=None):
        """(yR, dobsS, obs_count, dobs_const) of the dense or the obs_count form."""
        yR = self.yR if yR is None else yR
        if form == "dense":
            return yR, (self.dobsS if dobsS is None else dobsS), None, None
        return yR, None, (self.obs_count if counts is None else counts), self.dobs_const


def check_update(test, tag, D, A_out, b_out, want, twin):
    """(Am, bm) after a parameter update: rows 0 ... T-2 against the reference, the row T-1 still NaN, padding untouched (NaN)."""
    d, B, T = D.d, D.B, D.T
    for name, t, E, w, tw in (("A", A_out, d * d, want[0], twin[0]), ("b", b_out, d, want[1], twin[1])):
        raw = host(t)
        nat, own = np_vdp.unpack_nodes(raw, B, T, E, D.lv)
        assert np.all(np.isnan(raw[~own])) and np.all(np.isnan(nat[:, T - 1])), name
        held(test, f"{tag} {name}", nat[:, :T - 1].reshape(w.shape), w, tw)


# ---- the tests --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["full", "stab"])
@pytest.mark.parametrize("si", SHAPE_IX, ids=np_vdp.SHAPE_IDS)
@pytest.mark.parametrize("d", DIMS)
def test_vdp_to_ssm_and_naturals(amd, d, si, variant):
    """mfgm_packed_vdp_to_ssm and mfgm_packed_vdp_to_naturals (k_vdp_to_ssm<D>, k_vdp_to_naturals<D>): every node against the reference;
    NaN inputs come out as 1e-8 where the reference says so ("stab"); the last node's transition is zero."""
    test = "to_ssm_and_naturals"
    case, twin = reference(d, si, variant)
    D, r = Dev(amd, case), case.ref
    B, T, ET = D.B, D.T, d * (d + 1) // 2
    A, off, ch = D.out(d * d), D.out(d), D.out(ET)
    D.call("mfgm_packed_vdp_to_ssm", D.prm(), D.Am, D.bm, A, off, ch)
    gA = D.unpack(A, d * d)[0].reshape(B, T, d, d)
    held(test, "ssm A", gA, r.ssm[0], twin.ssm[0])
    held(test, "ssm off", D.unpack(off, d)[0], r.ssm[1], twin.ssm[1])
    held(test, "ssm chol", D.unpack(ch, ET)[0], np_vdp.tril_pack(r.ssm[2]), np_vdp.tril_pack(twin.ssm[2]))
    assert np.all(gA[:, T - 1] == 0.0)
    if variant == "stab":
        nanA, nanb = np.isnan(case.A), np.isnan(case.b)
        assert np.all(r.ssm[0][:, :T - 1][nanA] == LD(1e-8)) and np.all(gA[:, :T - 1][nanA] == 1e-8)
        assert np.all(D.unpack(off, d)[0][:, 1:][nanb] == 1e-8)
        assert np.abs(gA).max() <= 1.0 and np.abs(D.unpack(off, d)[0][:, 1:]).max() <= 1.0
    lin, dg, sb = D.out(d), D.out(ET), D.out(d * d)
    D.call("mfgm_packed_vdp_to_naturals", D.prm(), D.Am, D.bm, D.p0inv, D.p0lin, lin, dg, sb)
    held(test, "nat lin", D.unpack(lin, d)[0], r.nat[0], twin.nat[0])
    held(test, "nat diag", D.unpack(dg, ET)[0], np_vdp.tril_pack(r.nat[1]), np_vdp.tril_pack(twin.nat[1]))
    gs = D.unpack(sb, d * d)[0].reshape(B, T, d, d)
    held(test, "nat sub", gs, r.nat[2], twin.nat[2])
    assert np.all(gs[:, T - 1] == 0.0)


def held_energy(test, name, got, want, twin):
    """Per-chain energies: NaN exactly where the reference's is (the NaN drifts of "stab"), the rest by the rule."""
    fin = np.isfinite(np.asarray(want, dtype=np.float64))
    np.testing.assert_array_equal(np.isfinite(got), fin)
    if fin.any():
        held(test, name, got[fin], want[fin], twin[fin])


@pytest.mark.parametrize("variant", ["full", "stab"])
@pytest.mark.parametrize("si", SHAPE_IX, ids=np_vdp.SHAPE_IDS)
@pytest.mark.parametrize("d", DIMS)
def test_vdp_marginals(amd, d, si, variant):
    """mfgm_packed_vdp_marginals (k_vdp_marginals<D, 1>, k_vdp_marginals_scan<D>, k_vdp_marginals<D, 3>, k_sum_partials) with per-chain
    q(x0): means, covariances and e_over_dt (held to the reference esde on the reference marginals); with e_over_dt = NULL and no
    workspace the marginals are the same bit for bit."""
    test = "marginals"
    case, twin = reference(d, si, variant)
    D, r = Dev(amd, case), case.ref
    ET = d * (d + 1) // 2
    mu, Sig, e = D.out(d), D.out(ET), D.flat(D.B)
    D.call("mfgm_packed_vdp_marginals", D.prm(), D.Am, D.bm, D.q0_mu, D.q0_cov, mu, Sig, e, D.seg(), D.plan.ws)
    gm, raw_m = D.unpack(mu, d)
    gS, raw_S = D.unpack(Sig, ET)
    held(test, "m", gm, r.m, twin.m)
    held(test, "S", gS, np_vdp.tril_pack(r.S), np_vdp.tril_pack(twin.S))
    held_energy(test, "e_over_dt", host(e), r.e_fwd, twin.e_fwd)
    mu2, Sig2 = D.out(d), D.out(ET)
    D.call("mfgm_packed_vdp_marginals", D.prm(), D.Am, D.bm, D.q0_mu, D.q0_cov, mu2, Sig2, None, D.seg(), None)
    np.testing.assert_array_equal(host(mu2), raw_m)
    np.testing.assert_array_equal(host(Sig2), raw_S)


@pytest.mark.parametrize("kind", ["dw", "ou"])
@pytest.mark.parametrize("si", SHAPE_IX, ids=np_vdp.SHAPE_IDS)
@pytest.mark.parametrize("d", DIMS)
def test_vdp_esde(amd, d, si, kind):
    """mfgm_packed_vdp_esde (k_vdp_esde<D, true> / <D, false>) on the reference marginals, double-well and Ornstein-Uhlenbeck drifts
    with per-dimension parameters: e_over_dt, dE/dm / dt, dE/dS / dt on the nodes 0 ... T-2; the rows T-1 of gm, gS are not written
    (k_vdp_esde stores a node only when a transition starts there); without the gradient arrays the energy is held to the reference as
    well (the two instantiations contract their sums differently: 1 ulp apart on 2 of 70 chains)."""
    test = "esde"
    case, twin = reference(d, si, "full", kind)
    D, r = Dev(amd, case), case.ref
    T, ET = D.T, d * (d + 1) // 2
    e, gm, gS = D.flat(D.B), D.out(d), D.out(ET)
    D.call("mfgm_packed_vdp_esde", D.prm(), D.m, D.S, D.Am, D.bm, e, gm, gS, D.plan.ws)
    held(test, f"{kind} e_over_dt", host(e), r.e, twin.e)
    held(test, f"{kind} dE/dm", D.unpack(gm, d, T - 1)[0], r.gm, twin.gm)
    held(test, f"{kind} dE/dS", D.unpack(gS, ET, T - 1)[0], np_vdp.tril_pack(r.gS), np_vdp.tril_pack(twin.gS))
    e2 = D.flat(D.B)
    D.call("mfgm_packed_vdp_esde", D.prm(), D.m, D.S, D.Am, D.bm, e2, None, None, D.plan.ws)
    held(test, f"{kind} e_over_dt without the gradient arrays", host(e2), r.e, twin.e)


def run_lagrange(D, form, prm=None, **kw):
    d = D.d
    psi, lam = D.out(d * d), D.out(d)
    yR, dobsS, cnt, cst = D.jumps(form, **kw)
    D.call("mfgm_packed_vdp_lagrange", D.prm(prm), D.m, D.S, D.Am, D.bm, yR, dobsS, psi, lam, D.seg(), cnt, cst)
    return psi, lam


@pytest.mark.parametrize("variant", ["full", "noobs", "clip"])
@pytest.mark.parametrize("si", SHAPE_IX, ids=np_vdp.SHAPE_IDS)
@pytest.mark.parametrize("d", DIMS)
def test_vdp_lagrange(amd, d, si, variant):
    """mfgm_packed_vdp_lagrange (k_vdp_lagrange_products<D>, k_vdp_lagrange<D, 1>, k_vdp_lagrange_scan_wave<D>, k_vdp_lagrange<D, 3>) on the
    dense dobsS and on obs_count / dobs_const: psi, lam on the nodes 0 ... T-2 against the reference; the two jump forms agree bit for
    bit; the row T-1 and every entry no node owns keep the sentinel; other observations at node 0 and node T-1 change no output bit;
    the observations at node 1 and at node T-2 are read (the result is not the reference's without them)."""
    test = "lagrange"
    case, twin = reference(d, si, variant)
    D, r = Dev(amd, case), case.ref
    B, T = D.B, D.T
    res = {}
    for form in ("dense", "count"):
        psi, lam = run_lagrange(D, form)
        gp, raw_p = D.unpack(psi, d * d, T - 1)
        gl, raw_l = D.unpack(lam, d, T - 1)
        held(test, f"{variant} {form} psi", gp.reshape(r.psi.shape), r.psi, twin.psi)
        held(test, f"{variant} {form} lam", gl, r.lam, twin.lam)
        res[form] = (raw_p, raw_l, gp.reshape(r.psi.shape), gl)
    np.testing.assert_array_equal(res["dense"][0], res["count"][0])
    np.testing.assert_array_equal(res["dense"][1], res["count"][1])
    if variant == "noobs":
        return
    # nodes 0 and T-1 are not read: other observations there, the same bits
    rng = np.random.default_rng(d)
    yR, dobsS, counts = case.yR.copy(), case.dobsS.copy(), case.obs_count.copy()
    for node in (0, T - 1):
        yR[:, node] = rng.normal(size=(B, d))
        counts[:, node] += 3
        dobsS[:, node] = counts[:, node, None, None] * case.dobs_const
    for form in ("dense", "count"):
        psi, lam = run_lagrange(D, form, yR=D.pack(yR), dobsS=D.pack(np_vdp.tril_pack(dobsS)), counts=D.pack_counts(counts))
        np.testing.assert_array_equal(host(psi), res[form][0])
        np.testing.assert_array_equal(host(lam), res[form][1])
    # nodes 1 and T-2 are read
    if variant == "full" and T > 3:
        for node in (1, T - 2):
            wo = lagrange_without(d, si, node)
            for form in ("dense", "count"):
                assert np_vdp.rel_err(res[form][2], wo.psi) > 1e-3 and np_vdp.rel_err(res[form][3], wo.lam) > 1e-3, (node, form)


@pytest.mark.parametrize("lr", np_vdp.LRS)
@pytest.mark.parametrize("variant", ["full", "clip"])
@pytest.mark.parametrize("si", SHAPE_IX, ids=np_vdp.SHAPE_IDS)
@pytest.mark.parametrize("d", DIMS)
def test_vdp_update_param(amd, d, si, variant, lr):
    """mfgm_packed_vdp_update_param (k_vdp_update_param<D>) on the reference marginals and multipliers: (Am, bm) on the nodes 0 ... T-2;
    with clip > 0 psi / lam are overwritten by their clipped values (exactly: clipping does not round), otherwise left as they are."""
    test = "update_param"
    case, twin = reference(d, si, variant)
    D, r = Dev(amd, case), case.ref
    T = D.T
    psi, lam = D.rows(r.psi64.reshape(D.B, T - 1, -1)), D.rows(r.lam64)
    A, b = D.Am.clone(), D.bm.clone()
    D.call("mfgm_packed_vdp_update_param", D.prm(case.prm_m, lr), D.m, D.S, psi, lam, A, b)
    check_update(test, f"{variant} lr={lr}", D, A, b, r.upd[lr], twin.upd[lr])
    for name, t, E, want in (("psi", psi, d * d, r.upd[lr][2]), ("lam", lam, d, r.upd[lr][3])):
        nat, _ = np_vdp.unpack_nodes(host(t), D.B, T, E, D.lv)
        np.testing.assert_array_equal(nat[:, :T - 1].reshape(want.shape), want.astype(np.float64), err_msg=name)
        assert np.all(np.isnan(nat[:, T - 1]))
    if variant == "clip" and T > 2:
        assert np.abs(r.psi64).max() > case.prm_m.clip and np.abs(r.lam64).max() > case.prm_m.clip


@pytest.mark.parametrize("variant", ["full", "noobs", "clip"])
@pytest.mark.parametrize("si", SHAPE_IX, ids=np_vdp.SHAPE_IDS)
@pytest.mark.parametrize("d", DIMS)
def test_vdp_fused_routes(amd, d, si, variant):
    """Every fused route against the 80-bit reference of lagrange followed by update_param (lr = 0.3), never against another GPU route:
    mfgm_packed_vdp_lagrange_update (k_vdp_lagrange<D, 4>; obs_count form), mfgm_packed_vdp_lagrange_update0 (k_vdp_lagrange<D, 5>) in
    mode 0 (dense form), in mode 2 after mfgm_packed_vdp_marginals_products without the jump arguments and in mode 3 after that call
    with them (mode 3 on the marginals the call produced; its mu, Sig, e_over_dt are held to the reference too).  Then
    mfgm_packed_vdp_lagrange_update_final and mode 1 on restored (Am, bm) with the seg of the full call: bit-identical results."""
    test = "fused_routes"
    lr = 0.3
    case, twin = reference(d, si, variant)
    D, r = Dev(amd, case), case.ref
    B, T, ET = D.B, D.T, d * (d + 1) // 2
    want, tw = r.fused[lr], twin.fused[lr]
    prm = D.prm(lr=lr)

    def check_packed(tag, psi, lam):
        held(test, f"{tag} psi", D.unpack(psi, d * d, T - 1)[0].reshape(want[2].shape), want[2], tw[2])
        held(test, f"{tag} lam", D.unpack(lam, d, T - 1)[0], want[3], tw[3])

    def check_node0(tag, psi0, lam0):
        p0, l0 = host(psi0), host(lam0)
        if T == 2:                                   # the terminal values and nothing else
            np.testing.assert_array_equal(p0, np.broadcast_to(1e-10 * np.eye(d), (B, d, d)))
            np.testing.assert_array_equal(l0, np.zeros((B, d)))
            return
        held(test, f"{tag} psi(0)", p0, want[2][:, 0], tw[2][:, 0], scale=np.abs(want[2]).max())
        held(test, f"{tag} lam(0)", l0, want[3][:, 0], tw[3][:, 0], scale=np.abs(want[3]).max())

    # the kept-multipliers form
    A, b, psi, lam, seg = D.Am.clone(), D.bm.clone(), D.out(d * d), D.out(d), D.seg()
    D.call("mfgm_packed_vdp_lagrange_update", prm, D.m, D.S, A, b, *D.jumps("count")[:2], psi, lam, seg, *D.jumps("count")[2:])
    check_update(test, f"{variant} lagrange_update", D, A, b, want, tw)
    check_packed(f"{variant} lagrange_update", psi, lam)
    A2, b2, psi2, lam2 = D.Am.clone(), D.bm.clone(), D.out(d * d), D.out(d)
    D.call("mfgm_packed_vdp_lagrange_update_final", prm, D.m, D.S, A2, b2, *D.jumps("count")[:2], psi2, lam2, seg, *D.jumps("count")[2:])
    for x, y in ((A2, A), (b2, b), (psi2, psi), (lam2, lam)):
        np.testing.assert_array_equal(host(x), host(y))

    # node-0 multipliers, all passes
    A0, b0, psi0, lam0, seg0 = D.Am.clone(), D.bm.clone(), D.flat(B, d, d), D.flat(B, d), D.seg()
    D.call("mfgm_packed_vdp_lagrange_update0", prm, D.m, D.S, A0, b0, *D.jumps("dense")[:2], psi0, lam0, seg0, *D.jumps("dense")[2:], 0)
    check_update(test, f"{variant} update0 mode 0", D, A0, b0, want, tw)
    check_node0(f"{variant} update0 mode 0", psi0, lam0)
    A1, b1, psi1, lam1 = D.Am.clone(), D.bm.clone(), D.flat(B, d, d), D.flat(B, d)
    D.call("mfgm_packed_vdp_lagrange_update0", prm, D.m, D.S, A1, b1, *D.jumps("dense")[:2], psi1, lam1, seg0, *D.jumps("dense")[2:], 1)
    for x, y in ((A1, A0), (b1, b0), (psi1, psi0), (lam1, lam0)):
        np.testing.assert_array_equal(host(x), host(y))

    # the products call, then modes 2 and 3
    for mode, form in ((2, "count"), (3, "dense"), (3, "count")):
        mu, Sig, e, lseg = D.out(d), D.out(ET), D.flat(B), D.seg()
        jump = D.jumps(form) if mode == 3 else (None, None, None, None)
        D.call("mfgm_packed_vdp_marginals_products", D.prm(), D.Am, D.bm, D.q0_mu, D.q0_cov, mu, Sig, e, D.seg(), lseg, *jump, D.plan.ws)
        tag = f"{variant} products mode {mode} {form}"
        held(test, f"{tag} m", D.unpack(mu, d)[0], r.m, twin.m)
        held(test, f"{tag} S", D.unpack(Sig, ET)[0], np_vdp.tril_pack(r.S), np_vdp.tril_pack(twin.S))
        held(test, f"{tag} e_over_dt", host(e), r.e_fwd, twin.e_fwd)
        Ak, bk, psik, lamk = D.Am.clone(), D.bm.clone(), D.flat(B, d, d), D.flat(B, d)
        ms = (mu, Sig) if mode == 3 else (D.m, D.S)
        D.call("mfgm_packed_vdp_lagrange_update0", prm, *ms, Ak, bk, *D.jumps(form)[:2], psik, lamk, lseg, *D.jumps(form)[2:], mode)
        check_update(test, f"{tag} update0", D, Ak, bk, want, tw)
        check_node0(f"{tag} update0", psik, lamk)


@pytest.mark.parametrize("d", [4, 8])
def test_vdp_model_nonisotropic(amd, d):
    """VariationalMarkovGP at d = 4, 8 (B = 2, T = 41) with DoubleWellSDE(q = diag(distinct)) and a dense lower-triangular cholR,
    observations at the nodes 1, 2, 8, T-2: three iterations of the default fused route against the oracle (which takes a dense R)."""
    import torch
    from oracle import np_models, np_sde
    from tests.helpers import assert_close
    from vidp_amd import sde as gsde
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.vi_sde import VariationalMarkovGP
    B, T, dt = 2, 41, 0.01
    rng = np.random.default_rng(d)
    qd = 0.5 + np.arange(d) / d
    cholR = np.tril(0.2 * rng.normal(size=(d, d)), -1) + np.diag(0.4 + 0.3 * rng.random(d))
    grid = np.arange(T) * dt
    idx = np.array([1, 2, 8, T - 2])
    y = np.sign(rng.normal(size=(B, len(idx), d))) + 0.1 * rng.normal(size=(B, len(idx), d))
    init = (np.zeros(d), 0.5 * np.eye(d))
    plan = amd.Plan(B, T, d, R0=8, Rup=3)
    g = VariationalMarkovGP((grid[idx], dev(y)), gsde.DoubleWellSDE(torch.from_numpy(np.diag(qd))), grid, MultivariateGaussian(dev(cholR)),
                            prior_initial_state=init, plan=plan)
    os_ = [np_models.VariationalMarkovGP(idx, y[c], np_sde.DoubleWellSDE(np.diag(qd)), grid, np_models.MultivariateGaussianLik(cholR),
                                         *init, closed_form=True) for c in range(B)]
    for it in range(3):
        mS = g._forward_packed()
        g.update_lagrange_and_param(mS, lr=0.05)
        psi0, lam0 = (host(x) for x in g._mult0)
        g.update_initial_statistics(0.05)
        A, bb = host(plan.unpack(amd.FULL, g.A, T - 1)), host(plan.unpack(amd.VEC, g.b, T - 1))
        gm, gS = host(plan.unpack(amd.VEC, mS[0])), host(plan.unpack(amd.SYM, mS[1]))
        for c, o in enumerate(os_):
            m, S = o.forward_pass()
            assert_close(gm[c], m)
            assert_close(gS[c], S)
            o.update_lagrange(m, S)
            o.update_param(m, S, 0.05)
            assert_close(psi0[c], o.psi[0])
            assert_close(lam0[c], o.lam[0])
            assert_close(A[c], o.A)
            assert_close(bb[c], o.b)
            o.update_initial_statistics(0.05)
            assert_close(host(g.q0_mu)[c], o.q0_mu)
            assert_close(host(g.q0_chol)[c], o.q0_chol)
