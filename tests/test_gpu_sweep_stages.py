"""The staged (profiling) entry points of the lane-per-segment sweeps against the whole calls: mfgm_packed_factor_stage,
mfgm_packed_selinv_level, the only_level >= 0 forms of mfgm_packed_selinv_mom_s / _kl / _girsanov and mfgm_cq_selinv_kl,
mfgm_cq_factor_stage, mfgm_cq_factor_pair_stage and mfgm_cq_factor_pair_heads_stage.  Their contract (include/mfgm.h): a staged call
overwrites the outputs with identical values, so the stages of a sweep run one after the other ARE the sweep.  bench.py takes its
per-kernel figures from them.

Every comparison is bit for bit (assert_array_equal) on the entries a node owns; the outputs of the staged route go into
sentinel-filled arrays.  The dense staged calls launch one k_reduce / k_forward / k_backward per level, which run the lane-per-segment
bodies; the whole calls run levels of at most 16 segments per chain on the row bodies of the fused coarse kernels, which round
differently (test_coarse_row_bodies_agree_with_lane_bodies), so the dense tests set MFGM_COARSE_ROWS=0: the fused kernels then run
the bodies the per-level kernels run.  The staged cq calls launch the fused coarse kernels themselves and need no switch."""
import ctypes
import functools

import numpy as np
import pytest

from tests import np_cq
from tests import np_cq_heads as nh
from tests.helpers import random_dominant_btd
from tests.test_gpu_cq import CASES, SENT, amd, dev, device_state, host, make_plan, owned, sde_params, sentinel_like  # noqa: F401
from tests.test_gpu_cq_pair import LR, girsanov_level0_alt, kl_level0, sites

pytestmark = pytest.mark.gpu

STAGE_DIMS = [1, 3, 6, 8]
STAGE_CASES, STAGE_IDS = [CASES[0], CASES[2]], ["B3-T257", "B70-T9"]
LEVEL_SHAPE = (2, 1300, 2, 4)             # level 1 has 163 segments per chain: it keeps launches of its own in the whole calls


def _ptrs():
    from vidp_amd.packed import _ptr, _stream
    return _ptr, _stream


def level(plan, l):
    out = (ctypes.c_int * 4)()
    assert plan.lib.mfgm_plan_level(plan.h, l, out) == 0
    return tuple(out)                    # n, R, P, Lpad


def same(got, want, what, filled=True):
    got, want = [a if isinstance(a, np.ndarray) else host(a) for a in (got, want)]
    assert not (filled and np.any(got == SENT)), what
    np.testing.assert_array_equal(got, want, err_msg=what)


# ---- 1. dense: the stages one after the other are the whole call --------------------------------------------------------------------------
DENSE = [
    # B, T, d, R0, Rup
    (2, 5, 2, 2, 2),        # many tiny levels
    (3, 37, 3, 4, 3),       # ragged last segment, 3+ levels
    (2, 129, 6, 8, 8),
    (1, 150, 7, 10, 0),
    (1, 200, 8, 10, 0),
    (2, 1300, 3, 2, 4),     # level 1: 163 segments per chain, launches of its own in the whole call too
]


@pytest.mark.parametrize("with_rhs", [True, False], ids=["rhs", "norhs"])
@pytest.mark.parametrize("B,T,d,R0,Rup", DENSE)
def test_dense_stages_equal_whole(amd, rng, monkeypatch, B, T, d, R0, Rup, with_rhs):
    """mfgm_packed_factor_stage (stage 0 levels 0 .. K-1, stage 1 levels K .. 0) reproduces L, G, y of mfgm_packed_factor,
    mfgm_packed_selinv_level K .. 0 reproduces Sig, Sub, x of mfgm_packed_selinv, and a whole selected inverse after the staged
    factorisation (the coarse levels in the workspace are then the staged calls') equals the one after the whole factorisation."""
    _ptr, _stream = _ptrs()
    monkeypatch.setenv("MFGM_COARSE_ROWS", "0")
    diag, sub = random_dominant_btd(rng, (B,), T, d)
    plan = amd.Plan(B, T, d, R0=R0, Rup=Rup)
    K = plan.nlevels - 1
    assert K >= 1
    if T == 1300:
        assert level(plan, 1)[2] > 128 and K >= 2
    Dp, Sp = plan.pack(amd.SYM, dev(diag)), plan.pack(amd.FULL, dev(sub))
    rp = plan.pack(amd.VEC, dev(rng.normal(size=(B, T, d)))) if with_rhs else None
    kinds = [("L", amd.TRI, T), ("G", amd.FULL, T - 1)] + ([("y", amd.VEC, T)] if with_rhs else [])
    skinds = [("Sig", amd.SYM, T), ("Sub", amd.FULL, T - 1)] + ([("x", amd.VEC, T)] if with_rhs else [])
    unpack = lambda res, ks: {n: plan.unpack(k, res[n], nn) for n, k, nn in ks}

    f = plan.factor(Dp, Sp, rp, want_logdet=True, want_quad=with_rhs)
    plan.check_info()
    f_want = unpack(f, kinds)
    s_want = unpack(plan.selinv(f["L"], f["G"], f["y"], want_sub=True), skinds)

    g = {n: sentinel_like(plan.empty(k)) for n, k, _ in kinds}
    g.setdefault("y", None)
    for stage, levels in ((0, range(K)), (1, range(K, -1, -1))):
        for l in levels:
            rc = plan.lib.mfgm_packed_factor_stage(plan.h, stage, l, _ptr(Dp), _ptr(Sp), _ptr(rp), 1.0, 1.0, 1.0, _ptr(g["L"]), _ptr(g["G"]),
                                                   _ptr(g["y"]), _ptr(plan.ws), _ptr(plan.info), _stream())
            assert rc == 0, (stage, l)
    plan.check_info()
    for n, got in unpack(g, kinds).items():
        same(got, f_want[n], f"staged factor {n}")

    s = {n: sentinel_like(plan.empty(k)) for n, k, _ in skinds}
    s.setdefault("x", None)
    for l in range(K, -1, -1):
        rc = plan.lib.mfgm_packed_selinv_level(plan.h, l, _ptr(g["L"]), _ptr(g["G"]), _ptr(g["y"]), _ptr(s["Sig"]), _ptr(s["Sub"]), _ptr(s["x"]),
                                               _ptr(plan.ws), _stream())
        assert rc == 0, l
    for n, got in unpack(s, skinds).items():
        same(got, s_want[n], f"staged selected inverse {n}")

    out = {n: sentinel_like(plan.empty(k)) for n, k, _ in skinds}
    s2 = plan.selinv(g["L"], g["G"], g["y"], want_sub=True, out=out)
    for n, got in unpack(s2, skinds).items():
        same(got, s_want[n], f"whole selected inverse after the staged factorisation: {n}")


# ---- 2. the fused dense backward sweeps: only_level = K .. 1, then 0, against -1 ----------------------------------------------------------
@pytest.mark.parametrize("d", [3, 6])
def test_fused_dense_sweeps_by_level(amd, d, monkeypatch):
    """mfgm_packed_selinv_mom_s, mfgm_packed_selinv_kl and mfgm_packed_selinv_girsanov on a five-level plan: one call per level from the
    top down, the level-0 call last, against the whole call.  Inputs: the dense naturals of a cq state with its sites scattered in
    (as test_cq_equals_dense_entry_points makes them), factorised without the L_{t+1,t} output."""
    import torch
    _ptr, _stream = _ptrs()
    monkeypatch.setenv("MFGM_COARSE_ROWS", "0")
    st = state(d, STAGE_CASES[0])
    B, T = st.B, st.T
    plan = make_plan(amd, st)
    K = plan.nlevels - 1
    assert K >= 2
    cq = device_state(amd, plan, st)
    lin, diag, sub = plan.cq_unpack(cq)
    ids = dev((np.arange(B)[:, None] * T + st.obs_t).reshape(-1).astype(np.int64))
    plan.scatter_nodes(amd.VEC, lin, ids, dev(st.site_lin), accumulate=True)
    plan.scatter_nodes(amd.SYM, diag, ids, dev(np.broadcast_to(st.site_sym, (ids.numel(), d, d))), accumulate=True)
    prm = sde_params(amd, np_cq.sde_inputs(d, "dw"), LR)
    f = plan.factor(diag, sub, lin, aD=-2.0, aS=-1.0, aR=1.0, store_G=False)
    plan.check_info()
    L, y, lib, ws = f["L"], f["y"], plan.lib, plan.ws
    fresh = lambda *kinds: [sentinel_like(plan.empty(k)) for k in kinds]

    def mom_s(lv):
        Sig, x = fresh(amd.SYM, amd.VEC)
        mom = torch.full((3 * x.numel(),), SENT, dtype=torch.float64, device="cuda")
        for l in lv:
            assert lib.mfgm_packed_selinv_mom_s(plan.h, l, _ptr(L), _ptr(sub), -1.0, _ptr(y), _ptr(Sig), _ptr(x), _ptr(mom), _ptr(ws), _stream()) == 0
        return dict(Sig=plan.unpack(amd.SYM, Sig), x=plan.unpack(amd.VEC, x), mom=plan.unpack_moments(mom))

    def kl(lv):
        Sig, x = fresh(amd.SYM, amd.VEC)
        part = torch.full((B,), SENT, dtype=torch.float64, device="cuda")
        for l in lv:
            assert lib.mfgm_packed_selinv_kl(plan.h, l, _ptr(L), _ptr(sub), -1.0, _ptr(y), ctypes.byref(prm), _ptr(Sig), _ptr(x), _ptr(part),
                                             _ptr(ws), _stream()) == 0
        return dict(Sig=plan.unpack(amd.SYM, Sig), x=plan.unpack(amd.VEC, x), klpart=part)

    def girsanov(lv):
        n1, nd, ns = fresh(amd.VEC, amd.SYM, amd.FULL)
        for l in lv:
            assert lib.mfgm_packed_selinv_girsanov(plan.h, l, _ptr(L), _ptr(sub), -1.0, _ptr(y), ctypes.byref(prm), _ptr(lin), _ptr(diag),
                                                   _ptr(n1), _ptr(nd), _ptr(ns), _ptr(ws), _stream()) == 0
        return dict(lin=plan.unpack(amd.VEC, n1), diag=plan.unpack(amd.SYM, nd), sub=plan.unpack(amd.FULL, ns, T - 1))

    by_level = list(range(K, -1, -1))
    for name, sweep in (("mom_s", mom_s), ("kl", kl), ("girsanov", girsanov)):
        want = sweep([-1])
        got = sweep(by_level)
        for n in want:
            # (an entry of the moment array that neither route writes keeps its sentinel in both)
            same(got[n], want[n], f"{name} by level: {n}", filled=n != "mom")


# ---- 3. and 4. the cq routes -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def state(d, case, nxt=0):
    """State `nxt` of a case of tests/test_gpu_cq.py, or of a bare shape (no reference posterior is needed here)."""
    if len(case) == 2:
        si, variant = case
        st = np_cq.make_state(d, np_cq.SHAPES[si], sites=variant != "nosites", p0=variant != "nop0")
    else:
        st = np_cq.make_state(d, case)
    return np_cq.with_sites(st, nxt) if nxt else st


def cq_states(amd, d, case, n):
    sts = [state(d, case, k) for k in range(n)]
    plan = make_plan(amd, sts[0])
    cqs = [device_state(amd, plan, st) for st in sts]
    for cq in cqs[1:]:
        cq.dyn = cqs[0].dyn
    return sts, plan, cqs


def kl_by_level(amd, plan, cq, st, f, prm, levels):
    """mfgm_cq_selinv_kl once per entry of `levels` into one set of sentinel-filled outputs."""
    import torch
    d, n_tot = st.d, st.obs_t.size
    obs_mu = torch.full((n_tot + 2, d), SENT, dtype=torch.float64, device="cuda")
    obs_cov = torch.full((n_tot + 2, d, d), SENT, dtype=torch.float64, device="cuda")
    out = dict(Sig=sentinel_like(plan.empty(amd.SYM)), x=sentinel_like(plan.empty(amd.VEC)))
    for l in levels:
        s = plan.cq_selinv_kl(cq, f["L"], f["y"], prm, out=out, obs_mu=obs_mu, obs_cov=obs_cov, only_level=l)
    return dict(x=plan.unpack(amd.VEC, s["x"]), Sig=plan.unpack(amd.SYM, s["Sig"]), klpart=s["klpart"], obs_mu=obs_mu[:n_tot],
                obs_cov=obs_cov[:n_tot])


@pytest.mark.parametrize("case", STAGE_CASES, ids=STAGE_IDS)
@pytest.mark.parametrize("d", STAGE_DIMS)
def test_cq_stages_equal_whole(amd, d, case):
    """mfgm_cq_factor_stage 0 (level-0 reduce), 2 (the levels above), 1 (level-0 forward) reproduces (L, y) of mfgm_cq_factor;
    mfgm_cq_selinv_kl with only_level = 1 (the levels above alone) and then 0 equals the whole sweep."""
    _ptr, _stream = _ptrs()
    (st,), plan, (cq,) = cq_states(amd, d, case, 1)
    prm = sde_params(amd, np_cq.sde_inputs(d, "dw"))
    f = plan.cq_factor(cq)
    want = owned(st, dict(L=f["L"], y=f["y"]))
    s_want = kl_by_level(amd, plan, cq, st, f, prm, [-1])
    g = dict(L=sentinel_like(plan.empty(amd.TRI)), y=sentinel_like(plan.empty(amd.VEC)))
    for stage in (0, 2, 1):
        assert plan.lib.mfgm_cq_factor_stage(plan.h, stage, ctypes.byref(cq.struct()), _ptr(g["L"]), _ptr(g["y"]), _ptr(plan.ws), _ptr(plan.info),
                                             _stream()) == 0
    plan.check_info()
    got = owned(st, g)
    for n in ("L", "y"):
        same(got[n], want[n], f"staged cq factor {n}")
    s = kl_by_level(amd, plan, cq, st, g, prm, [1, 0])
    for n in s_want:
        same(s[n], s_want[n], f"cq KL sweep by level: {n}")


def pair_by_stage(amd, plan, cqa, cqb, stride=None):
    """The four stages of the pair call (0 level-0 reduces, 2 joint up phase, 1 level-0 forward pair, 3 joint backward pass) into
    sentinel-filled factor arrays."""
    _ptr, _stream = _ptrs()
    a, b = cqa.struct(), cqa.struct()
    b.site_lin, b.site_sym = cqb.site_lin.data_ptr(), cqb.site_sym.data_ptr()
    fa, fb = [dict(L=sentinel_like(plan.empty(amd.TRI)), y=sentinel_like(plan.empty(amd.VEC))) for _ in range(2)]
    for stage in (0, 2, 1, 3):
        if stride is None:
            rc = plan.lib.mfgm_cq_factor_pair_stage(plan.h, stage, ctypes.byref(a), ctypes.byref(b), _ptr(fa["L"]), _ptr(fa["y"]), _ptr(fb["L"]),
                                                    _ptr(fb["y"]), _ptr(plan.ws), _ptr(plan.info), _stream())
        else:
            scratch = plan._heads_scratch(stride)
            rc = plan.lib.mfgm_cq_factor_pair_heads_stage(plan.h, stage, stride, ctypes.byref(a), ctypes.byref(b), _ptr(fa["L"]), _ptr(fa["y"]),
                                                          _ptr(fb["L"]), _ptr(fb["y"]), _ptr(scratch), scratch.numel(), _ptr(plan.ws),
                                                          _ptr(plan.info), _stream())
        assert rc == 0, stage
    return fa, fb


def check_pair_stages(amd, d, sts, plan, cqs, stride=None):
    st = sts[0]
    sd = np_cq.sde_inputs(d, "dw")
    prm0, prm = sde_params(amd, sd), sde_params(amd, sd, LR)
    fa, fb = plan.cq_factor_pair(cqs[0], sites(cqs[1]), head_stride=stride)
    want = [owned(st, dict(L=f["L"], y=f["y"])) for f in (fa, fb)]
    s_want = kl_level0(amd, plan, cqs[0], st, fa, prm0)
    g_want = girsanov_level0_alt(plan, cqs[1], fb, prm)
    ga, gb = pair_by_stage(amd, plan, cqs[0], cqs[1], stride)
    plan.check_info()
    for which, g, w in (("A", ga, want[0]), ("B", gb, want[1])):
        got = owned(st, g)
        for n in ("L", "y"):
            same(got[n], w[n], f"staged pair {which} {n}")
    s = kl_level0(amd, plan, cqs[0], st, ga, prm0)
    for n in ("x", "Sig", "klpart", "obs_mu", "obs_cov"):
        np.testing.assert_array_equal(s[n], s_want[n], err_msg=f"level-0 KL sweep after the staged pair: {n}")
    np.testing.assert_array_equal(girsanov_level0_alt(plan, cqs[1], gb, prm), g_want, err_msg="level-0 Girsanov sweep after the staged pair")
    plan.check_info()


@pytest.mark.parametrize("d,case", [(d, c) for c in STAGE_CASES for d in STAGE_DIMS] + [(3, LEVEL_SHAPE), (8, LEVEL_SHAPE)],
                         ids=[f"d{d}-{i}" for i in STAGE_IDS for d in STAGE_DIMS] + ["d3-B2-T1300", "d8-B2-T1300"])
def test_cq_pair_stages_equal_whole(amd, d, case):
    """mfgm_cq_factor_pair_stage 0, 2, 1, 3 reproduces (L, y, L2, y2) of mfgm_cq_factor_pair, and the level-0 KL sweep on A and the
    level-0 Girsanov sweep on B after it (on the separator marginals stage 3 left) equal those after the whole call."""
    sts, plan, cqs = cq_states(amd, d, case, 2)
    if case == LEVEL_SHAPE:
        assert level(plan, 1)[2] > 128 and plan.nlevels >= 3
    check_pair_stages(amd, d, sts, plan, cqs)


def test_cq_pair_heads_stages_equal_whole(amd):
    """The same through mfgm_cq_factor_pair_heads_stage (stage 0: the shared interior elimination and the two head reduces)."""
    d, shape = 3, nh.SHAPES[0]
    sts = [nh.make_state(d, shape)]
    sts.append(np_cq.with_sites(sts[0], 1))
    plan = make_plan(amd, sts[0])
    assert plan.R % sts[0].q == 0
    cqs = [device_state(amd, plan, st) for st in sts]
    cqs[1].dyn = cqs[0].dyn
    check_pair_stages(amd, d, sts, plan, cqs, stride=sts[0].q)


# ---- 5. the argument check of the staged pair call ------------------------------------------------------------------------------------------
def test_cq_pair_stage_argument_errors(amd):
    """mfgm_cq_factor_pair_stage with a second state whose d_off, s_off or p0_off is not the first one's (the two must be one dyn with
    two sets of sites, as for mfgm_cq_factor_pair): reported, nothing launched."""
    import torch
    _ptr, _stream = _ptrs()
    d = 3
    sts, plan, cqs = cq_states(amd, d, STAGE_CASES[0], 2)
    other_p0 = cqs[0].p0_off.clone()
    arrs = [sentinel_like(plan.empty(k)) for k in (amd.TRI, amd.VEC, amd.TRI, amd.VEC)]

    def raw(stage, **changed):
        a, b = cqs[0].struct(), cqs[0].struct()
        b.site_lin, b.site_sym = cqs[1].site_lin.data_ptr(), cqs[1].site_sym.data_ptr()
        for name, v in changed.items():
            setattr(b, name, v)
        return plan.lib.mfgm_cq_factor_pair_stage(plan.h, stage, ctypes.byref(a), ctypes.byref(b), *[_ptr(t) for t in arrs], _ptr(plan.ws),
                                                  _ptr(plan.info), _stream())
    for changed in (dict(d_off=cqs[0].d_off + 0.5), dict(s_off=cqs[0].s_off + 0.5), dict(p0_off=other_p0.data_ptr())):
        for stage in range(4):
            assert raw(stage, **changed) == 1, (changed, stage)
    torch.cuda.synchronize()
    assert all(bool((t == SENT).all()) for t in arrs)
    for stage in (0, 2, 1, 3):
        assert raw(stage) == 0
    plan.check_info()
    torch.cuda.synchronize()
    assert not any(bool((t == SENT).all()) for t in arrs)
