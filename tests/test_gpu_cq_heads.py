"""mfgm_cq_factor_pair_heads: the pair of factorisations of tests/test_gpu_cq_pair.py for observations on a regular grid, the two
level-0 reduces sharing the elimination of everything but the observed nodes (k_reduce_cq_interior once, k_reduce_cq_heads per site
set); and CVISitesSDE on that route.

States come from tests/np_cq_heads.py: observations on multiples of q, every chain on its own subset of the heads (shapes and what
each is there for: np_cq_heads.SHAPES).  The elimination ORDER differs from mfgm_cq_factor's, so nothing is bit-identical here: the
factors are held to plain mfgm_cq_factor within 1e-12 of the array's largest entry (the bound test_cq_pipelined_forms uses for a
reordered reduce), what the level-0 sweeps make of them to the 80-bit reference of tests/np_cq.py under that module's rule,
max(8 x yardstick, 64 eps)."""
import functools

import numpy as np
import pytest

from tests import np_cq
from tests import np_cq_heads as nh
from tests.test_gpu_cq import SENT, amd, check_marginals, dev, device_state, held, host, make_plan, owned, sde_params, sentinel_like  # noqa: F401
from tests.test_gpu_cq_pair import LR, girsanov_level0_alt, kl_host, kl_level0, sites

pytestmark = pytest.mark.gpu

CASES = [(d, s) for s in nh.SHAPES for d in nh.DIMS]
IDS = [f"{i}-d{d}" for i in nh.SHAPE_IDS for d in nh.DIMS]
REORDER = 1e-12


@functools.lru_cache(maxsize=None)
def reference(d, shape, nxt=0):
    st = nh.make_state(d, shape)
    if nxt:
        st = np_cq.with_sites(st, nxt)
    return dict(st=st, ref=np_cq.posterior(st), orc=np_cq.posterior_fp64(st))


@functools.lru_cache(maxsize=None)
def reference_girsanov(d, shape, nxt):
    r = reference(d, shape, nxt)
    sd = np_cq.sde_inputs(d, "dw")
    args = (r["st"], sd.alpha, sd.beta, sd.qd, sd.dt, sd.init_mu, sd.init_cov)
    return (np_cq.kl_and_girsanov(*args, lr=[LR], post=r["ref"]).dyn_out[0], np_cq.kl_and_girsanov(*args, lr=[LR], post=r["orc"]).dyn_out[0])


def states(amd, d, shape, n):
    refs = [reference(d, shape, k) for k in range(n)]
    plan = make_plan(amd, refs[0]["st"])
    assert plan.R % shape[4] == 0
    cqs = [device_state(amd, plan, r["st"]) for r in refs]
    for cq in cqs[1:]:
        cq.dyn = cqs[0].dyn
    return refs, plan, cqs


def pair_heads(plan, cqa, cqb, q):
    out = [dict(L=sentinel_like(plan.empty(3)), y=sentinel_like(plan.empty(0))) for _ in range(2)]
    return plan.cq_factor_pair(cqa, sites(cqb), out=out[0], out2=out[1], head_stride=q)


def close(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert not np.any(got == SENT), what
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"  {what}: largest difference {err:.3e} of the largest entry")
    assert err <= REORDER, (what, err)


def close_factor(st, got, want, names, what):
    got, want = owned(st, {n: got[n] for n in names}), owned(st, {n: want[n] for n in names})
    for n in names:
        close(f"{what} {n} against mfgm_cq_factor", got[n], want[n])


@pytest.mark.parametrize("d,shape", CASES, ids=IDS)
def test_heads_pair_equals_plain_factor(amd, d, shape):
    """(L, y, logdet) = mfgm_cq_factor on sites A and (L2, y2) = mfgm_cq_factor on sites B."""
    refs, plan, cqs = states(amd, d, shape, 2)
    st = refs[0]["st"]
    plain = [plan.cq_factor(cq) for cq in cqs]
    fa, fb = pair_heads(plan, cqs[0], cqs[1], st.q)
    plan.check_info()
    close_factor(st, fa, plain[0], ("L", "y", "logdet"), "A")
    close_factor(st, fb, plain[1], ("L", "y"), "B")


@pytest.mark.parametrize("d,shape", CASES, ids=IDS)
def test_heads_pair_downstream_sweeps(amd, d, shape):
    """The level-0 KL sweep on A and the level-0 Girsanov sweep on B through the second coarse copy, against the 80-bit reference."""
    test = "heads_downstream"
    refs, plan, cqs = states(amd, d, shape, 2)
    st = refs[0]["st"]
    sd = np_cq.sde_inputs(d, "dw")
    fa, fb = pair_heads(plan, cqs[0], cqs[1], st.q)
    s = kl_level0(amd, plan, cqs[0], st, fa, sde_params(amd, sd))
    g = girsanov_level0_alt(plan, cqs[1], fb, sde_params(amd, sd, LR))
    plan.check_info()
    check_marginals(test, st, refs[0], fa, s)
    got, _ = np_cq.unpack_nodes(g, st.B, st.T, 3 * d, st.levels[0])
    assert not np.any(got == SENT)
    want, orc = reference_girsanov(d, shape, 1)
    T = st.T
    for name, sl, tt in (("lin", slice(0, d), T), ("diag", slice(d, 2 * d), T), ("sub", slice(2 * d, 3 * d), T - 1)):
        held(test, f"girsanov on B {name}", got[:, :tt, sl], want[:, :tt, sl], orc[:, :tt, sl])
    np.testing.assert_array_equal(got[:, T - 1, 2 * d:], st.dyn[:, T - 1, 2 * d:])


@pytest.mark.parametrize("d,shape", CASES, ids=IDS)
def test_heads_pair_calls_in_a_row_and_a_plain_call_between(amd, d, shape):
    """Three calls in a row with the site sets rotating, (A, B) = (0, 1), (1, 2), (2, 0): each call parks over what the one before
    left and writes either copy of the coarse levels in turn.  Then a plain mfgm_cq_factor of the third state between a call and its
    sweeps, as in test_gpu_cq_pair: the first copy is then state 2's, the second still gives B's Girsanov sweep."""
    refs, plan, cqs = states(amd, d, shape, 3)
    st = refs[0]["st"]
    sd = np_cq.sde_inputs(d, "dw")
    prm0, prm = sde_params(amd, sd), sde_params(amd, sd, LR)
    plain = [plan.cq_factor(cq) for cq in cqs]
    want_kl, want_g = [], []
    for cq in cqs:
        f = plan.cq_factor(cq)
        s = plan.cq_selinv_kl(cq, f["L"], f["y"], prm0)
        out = sentinel_like(cq.dyn)
        plan.cq_selinv_girsanov(cq, f["L"], f["y"], prm, out)
        want_kl.append(kl_host(amd, plan, s))
        want_g.append(host(out))
    own_dyn = np_cq.unpack_nodes(want_g[0], st.B, st.T, 3 * d, st.levels[0])[1]
    for a, b in ((0, 1), (1, 2), (2, 0)):
        fa, fb = pair_heads(plan, cqs[a], cqs[b], st.q)
        close_factor(st, fa, plain[a], ("L", "y", "logdet"), f"A = {a}")
        close_factor(st, fb, plain[b], ("L", "y"), f"B = {b}")
        s = kl_host(amd, plan, plan.cq_selinv_kl(cqs[a], fa["L"], fa["y"], prm0, only_level=0))
        for n in ("x", "Sig", "klpart"):
            close(f"KL sweep on A = {a}: {n}", s[n], want_kl[a][n])
        close(f"Girsanov sweep on B = {b}", girsanov_level0_alt(plan, cqs[b], fb, prm)[own_dyn], want_g[b][own_dyn])
    fa, fb = pair_heads(plan, cqs[0], cqs[1], st.q)
    f2 = plan.cq_factor(cqs[2])
    s = kl_host(amd, plan, plan.cq_selinv_kl(cqs[2], f2["L"], f2["y"], prm0))
    for n in ("x", "Sig", "klpart"):
        np.testing.assert_array_equal(s[n], want_kl[2][n], err_msg=f"KL sweep after a plain factor: {n}")
    close("Girsanov sweep on B after a plain factor", girsanov_level0_alt(plan, cqs[1], fb, prm)[own_dyn], want_g[1][own_dyn])
    plan.check_info()


def test_heads_pair_argument_errors(amd):
    """stride < 2, a stride that does not divide the segment length (and the scratch size of those), a scratch array that is too
    small, a plan without the second coarse copy: reported, nothing launched."""
    d, shape = 3, nh.SHAPES[0]
    refs, plan, cqs = states(amd, d, shape, 2)
    st = refs[0]["st"]
    E = 2 * (d * (d + 1) // 2) + 2 * d + d * d
    assert plan.R == 8
    assert plan.lib.mfgm_cq_heads_scratch_doubles(plan.h, 4) == plan.Lpad * 2 * E
    assert plan.lib.mfgm_cq_heads_scratch_doubles(plan.h, 8) == plan.Lpad * E
    for bad in (-4, 0, 1, 3, 5, 16):
        assert plan.lib.mfgm_cq_heads_scratch_doubles(plan.h, bad) == 0
        with pytest.raises(ValueError, match="mfgm_cq_factor_pair_heads"):
            pair_heads(plan, cqs[0], cqs[1], bad)
    # a scratch array one double short of what the stride needs (as one sized for stride 8 would be for stride 4), and a plan without
    # the second copy of the coarse levels (one level): refused before anything is launched, the factor arrays keep their sentinels
    import ctypes
    import torch
    from vidp_amd.packed import _ptr, _stream

    def raw(pl, stride, scratch, size, L, y, L2, y2):
        a, b = cqs[0].struct(), cqs[0].struct()
        b.site_lin, b.site_sym = cqs[1].site_lin.data_ptr(), cqs[1].site_sym.data_ptr()
        return pl.lib.mfgm_cq_factor_pair_heads(pl.h, stride, ctypes.byref(a), ctypes.byref(b), _ptr(L), _ptr(y), None, None, _ptr(L2),
                                                _ptr(y2), _ptr(scratch), size, _ptr(pl.ws), _ptr(pl.info), _stream())
    need = plan.Lpad * 2 * E
    scratch = torch.empty(need, dtype=torch.float64, device="cuda")
    arrs = [sentinel_like(plan.empty(k)) for k in (3, 0, 3, 0)]
    assert raw(plan, 4, scratch, need - 1, *arrs) == 1
    assert raw(plan, 4, scratch, plan.lib.mfgm_cq_heads_scratch_doubles(plan.h, 8), *arrs) == 1
    small = amd.Plan(1, 8, d, R0=8)
    assert small.nlevels == 1
    assert raw(small, 4, scratch, need, *arrs) == 1
    torch.cuda.synchronize()
    assert all(bool((t == SENT).all()) for t in arrs)
    assert raw(plan, 4, scratch, need, *arrs) == 0
    plan.check_info()
    # a good call still works after the refused ones (the scratch array is sized again for its stride)
    plain = plan.cq_factor(cqs[0])
    fa, _ = pair_heads(plan, cqs[0], cqs[1], st.q)
    plan.check_info()
    close_factor(st, fa, plain, ("L", "y", "logdet"), "after refused calls")


def test_cvi_dp_heads_pair_steps_equal_unpipelined(amd, rng):
    """CVISitesSDE with observations at arange(20, T, 20) and segments of 40 nodes: the pair route takes the new entry (stride 20) on
    every call.  The program of test_cvi_dp_pair_steps_equal_unpipelined against the same model with the pipelining switched off."""
    import torch
    from vidp_amd import sde as gsde
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.variational_cvi_sde import CVISitesSDE
    B, T, d, dt = 3, 1200, 3, 0.01
    grid = np.arange(T) * dt
    idx = np.arange(20, T, 20)
    y = np.sign(rng.normal(size=(B, len(idx), d))) + 0.1 * rng.normal(size=(B, len(idx), d))
    cholR = 0.3 * np.eye(d)

    def make(pipe):
        m = CVISitesSDE(gsde.DoubleWellSDE(torch.eye(d, dtype=torch.float64)), grid, (grid[idx], dev(y)), MultivariateGaussian(dev(cholR)),
                        prior_initial_state=(np.zeros(d), np.eye(d)), plan=amd.Plan(B, T, d, R0=40, Rup=4))
        m.pipelined, m.pipe_pair, m.pipe_two_streams, m.pair_heads = pipe, True, False, True
        m.pipeline_min_nodes = 0
        return m
    a, b = make(False), make(True)
    assert b._cq_state() is not None and b.plan.R == 40 and b._pair_head_stride() == 20
    strides, alt_sweeps = [], []
    pair, sweep = b.plan.cq_factor_pair, b.plan.cq_selinv_girsanov
    b.plan.cq_factor_pair = lambda *args, **kw: (strides.append(kw.get("head_stride")), pair(*args, **kw))[1]
    b.plan.cq_selinv_girsanov = lambda *args, **kw: (alt_sweeps.append(bool(kw.get("alt"))), sweep(*args, **kw))[1]

    def state(m):
        cq = m._cq_state()
        return [host(t) for t in (cq.dyn, m.data_nat1, cq.site_sym, m.fx_mus_obs, m.fx_covs_obs)]

    prog = [("s", 0.5, 0.1)] * 4 + [("e",), ("s", 0.3, 0.1), ("s", 0.3, 0.1), ("snap",), ("s", 0.3, 0.2), ("s", 0.3, 0.2), ("restore",),
                                    ("s", 0.3, 0.2), ("s", 0.3, 0.2)]
    got, want, snaps = [], [], {}
    for op in prog:
        for m, out in ((a, want), (b, got)):
            if op[0] == "s":
                m.update_data_sites(op[1])
                m.update_girsanov_sites(op[2])
            elif op[0] == "snap":
                snaps[id(m)] = m.snapshot()
                continue
            elif op[0] == "restore":
                m.restore(snaps[id(m)])
            out.append(host(m.classic_elbo_per_trajectory()))
    b.plan.check_info()
    assert alt_sweeps == [False, True, True, True, False, True, True, True, True, True], alt_sweeps
    assert b._ahead.consumed == sum(alt_sweeps)
    # every pair call went through mfgm_cq_factor_pair_heads: the stride was passed and the plan holds that entry's scratch array
    assert len(strides) >= sum(alt_sweeps) and set(strides) == {20}, strides
    assert b.plan._heads_buf[0] == 20 and b.plan._heads_buf[1].numel() == b.plan.lib.mfgm_cq_heads_scratch_doubles(b.plan.h, 20)
    assert not hasattr(a.plan, "_heads_buf")
    got, want = np.array(got), np.array(want)
    np.testing.assert_allclose(got, want, rtol=1e-12)
    np.testing.assert_array_equal(got[-3:], got[-6:-3])
    for x, z, name in zip(state(b), state(a), ("dyn", "site_lin", "site_sym", "fx_mus_obs", "fx_covs_obs")):
        np.testing.assert_allclose(x, z, rtol=1e-12, atol=1e-12 * np.abs(z).max(), err_msg=name)
