"""mfgm_cq_factor_pair and mfgm_cq_selinv_girsanov_alt: two factorisations of one dyn (two sets of observation sites) whose levels above
the finest one run once at double width, the second in the workspace's second copy of those levels; and CVISitesSDE on that route.

Kernels launched here: k_forward_pair_cq<D, 0> (D = 1 ... 6; <D, 1> at D = 3, 6 in test_pair_cache_policy), k_coarse_factor_pair,
k_coarse_backward_pair, k_reduce_cq twice, and at D = 7, 8 k_forward_cq twice; k_reduce_pair / k_forward_pair / k_backward_pair (a level
above the finest one with more than 128 segments per chain keeps a launch of its own) in test_pair_level_launches.

Every body is the one the single route runs, on the same inputs in the same order: the results are held to be BIT-IDENTICAL to plain
mfgm_cq_factor / mfgm_cq_selinv_kl / mfgm_cq_selinv_girsanov wherever a test compares the two (the issue's bound is 1e-12 of the
largest entry; both are asserted), and to the 80-bit reference of tests/np_cq.py under that module's bound, max(8 x yardstick, 64 eps),
downstream."""
import functools

import numpy as np
import pytest

from tests import np_cq
from tests.test_gpu_cq import (CASE_IDS, CASES, DIMS, SENT, amd, check_marginals, dev, device_state, held, host, make_plan,  # noqa: F401
                               owned, reference, sde_params, sentinel_like)

pytestmark = pytest.mark.gpu

PAIR_CASES, PAIR_IDS = CASES[:3], CASE_IDS[:3]
LR = 0.3


@functools.lru_cache(maxsize=None)
def reference_girsanov(d, case, nxt):
    """dyn_out of the Girsanov sweep at lr = LR for state `nxt` of the case: (80-bit reference, fp64 oracle)."""
    r = reference(d, case, nxt)
    sd = np_cq.sde_inputs(d, "dw")
    args = (r["st"], sd.alpha, sd.beta, sd.qd, sd.dt, sd.init_mu, sd.init_cov)
    return (np_cq.kl_and_girsanov(*args, lr=[LR], post=r["ref"]).dyn_out[0], np_cq.kl_and_girsanov(*args, lr=[LR], post=r["orc"]).dyn_out[0])


def states(amd, d, case, n):
    refs = [reference(d, case, k) for k in range(n)]
    plan = make_plan(amd, refs[0]["st"])
    cqs = [device_state(amd, plan, r["st"]) for r in refs]
    for cq in cqs[1:]:
        cq.dyn = cqs[0].dyn                          # one resident state, n sets of data sites
    return refs, plan, cqs


def sites(cq):
    return cq.site_lin, cq.site_sym


def pair(plan, cqa, cqb):
    """cq_factor_pair into sentinel-filled factor arrays."""
    out = [dict(L=sentinel_like(plan.empty(3)), y=sentinel_like(plan.empty(0))) for _ in range(2)]
    return plan.cq_factor_pair(cqa, sites(cqb), out=out[0], out2=out[1])


def same_factor(st, got, want, names, what):
    got, want = owned(st, {n: got[n] for n in names}), owned(st, {n: want[n] for n in names})
    for n in names:
        a, b = got[n], want[n]
        assert not np.any(a == SENT), (what, n)
        print(f"  pair {what} {n}: largest difference from mfgm_cq_factor {np.abs(a - b).max() / np.abs(b).max():.3e} of the largest entry")
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), (what, n)
        np.testing.assert_array_equal(a, b, err_msg=f"{what} {n}")


def kl_level0(amd, plan, cq, st, f, prm):
    """The level-0 KL sweep alone (only_level = 0: the separator marginals are what the pair call's joint coarse backward pass left),
    in the form check_marginals takes."""
    import torch
    d, n_tot = st.d, st.obs_t.size
    obs_mu = torch.full((n_tot + 2, d), SENT, dtype=torch.float64, device="cuda")
    obs_cov = torch.full((n_tot + 2, d, d), SENT, dtype=torch.float64, device="cuda")
    out = dict(Sig=sentinel_like(plan.empty(amd.SYM)), x=sentinel_like(plan.empty(amd.VEC)))
    s = plan.cq_selinv_kl(cq, f["L"], f["y"], prm, out=out, obs_mu=obs_mu, obs_cov=obs_cov, only_level=0)
    return dict(klpart=host(s["klpart"]), obs_mu=host(obs_mu), obs_cov=host(obs_cov), x=host(plan.unpack(amd.VEC, s["x"])),
                Sig=host(plan.unpack(amd.SYM, s["Sig"])), raw_x=host(s["x"]), raw_Sig=host(s["Sig"]))


def kl_host(amd, plan, s):
    """Host copies of a KL sweep's results; of the packed marginal arrays (made with torch.empty) only the entries a node owns."""
    return dict(x=host(plan.unpack(amd.VEC, s["x"])), Sig=host(plan.unpack(amd.SYM, s["Sig"])), klpart=host(s["klpart"]))


def girsanov_level0_alt(plan, cq, f2, prm):
    out = sentinel_like(cq.dyn)
    plan.cq_selinv_girsanov(cq, f2["L"], f2["y"], prm, out, only_level=0, alt=True)
    return host(out)


@pytest.mark.parametrize("case", PAIR_CASES, ids=PAIR_IDS)
@pytest.mark.parametrize("d", DIMS)
def test_pair_equals_plain_factor(amd, d, case):
    """(L, y, logdet) of the pair call = mfgm_cq_factor on sites A, (L2, y2) = mfgm_cq_factor on sites B: d <= 6 the two-wavefront
    kernel, d = 7, 8 two forward sweeps."""
    refs, plan, cqs = states(amd, d, case, 2)
    st = refs[0]["st"]
    plain = [plan.cq_factor(cq) for cq in cqs]
    fa, fb = pair(plan, cqs[0], cqs[1])
    plan.check_info()
    same_factor(st, fa, plain[0], ("L", "y", "logdet"), "A")
    same_factor(st, fb, plain[1], ("L", "y"), "B")


@pytest.mark.parametrize("case", PAIR_CASES, ids=PAIR_IDS)
@pytest.mark.parametrize("d", DIMS)
def test_pair_downstream_sweeps(amd, d, case):
    """The level-0 KL sweep on A and the level-0 Girsanov sweep on B through the second coarse copy, both on the separator marginals
    the pair call left, against the 80-bit reference."""
    test = "pair_downstream"
    refs, plan, cqs = states(amd, d, case, 2)
    st = refs[0]["st"]
    sd = np_cq.sde_inputs(d, "dw")
    fa, fb = pair(plan, cqs[0], cqs[1])
    s = kl_level0(amd, plan, cqs[0], st, fa, sde_params(amd, sd))
    g = girsanov_level0_alt(plan, cqs[1], fb, sde_params(amd, sd, LR))
    plan.check_info()
    check_marginals(test, st, refs[0], fa, s)
    got, _ = np_cq.unpack_nodes(g, st.B, st.T, 3 * d, st.levels[0])
    assert not np.any(got == SENT)
    want, orc = reference_girsanov(d, case, 1)
    T = st.T
    for name, sl, tt in (("lin", slice(0, d), T), ("diag", slice(d, 2 * d), T), ("sub", slice(2 * d, 3 * d), T - 1)):
        held(test, f"girsanov on B {name}", got[:, :tt, sl], want[:, :tt, sl], orc[:, :tt, sl])
    np.testing.assert_array_equal(got[:, T - 1, 2 * d:], st.dyn[:, T - 1, 2 * d:])


@pytest.mark.parametrize("case", PAIR_CASES, ids=PAIR_IDS)
@pytest.mark.parametrize("d", [1, 3, 6, 8])
def test_pair_calls_in_a_row_and_a_plain_call_between(amd, d, case):
    """Three pair calls in a row on three site sets, (A, B) = (0, 1), (1, 2), (2, 0): every site set is factorised in either copy of
    the coarse levels in turn, over what the call before left there.  Then a plain mfgm_cq_factor of the third state between a pair
    call and its sweeps: it overwrites the first copy, so a KL sweep on ITS factor must find its own separator marginals there (not
    those of the pair's A), while (L2, y2) and the second copy -- which it does not touch -- still give B's Girsanov sweep."""
    refs, plan, cqs = states(amd, d, case, 3)
    st = refs[0]["st"]
    sd = np_cq.sde_inputs(d, "dw")
    prm0, prm = sde_params(amd, sd), sde_params(amd, sd, LR)
    plain = [plan.cq_factor(cq) for cq in cqs]
    # what the single route gives downstream
    want_kl, want_g = [], []
    for cq in cqs:
        f = plan.cq_factor(cq)
        s = plan.cq_selinv_kl(cq, f["L"], f["y"], prm0)
        out = sentinel_like(cq.dyn)
        plan.cq_selinv_girsanov(cq, f["L"], f["y"], prm, out)
        want_kl.append(kl_host(amd, plan, s))
        want_g.append(host(out))
    for a, b in ((0, 1), (1, 2), (2, 0)):
        fa, fb = pair(plan, cqs[a], cqs[b])
        same_factor(st, fa, plain[a], ("L", "y", "logdet"), f"A = {a}")
        same_factor(st, fb, plain[b], ("L", "y"), f"B = {b}")
        s = kl_host(amd, plan, plan.cq_selinv_kl(cqs[a], fa["L"], fa["y"], prm0, only_level=0))
        for n in ("x", "Sig", "klpart"):
            np.testing.assert_array_equal(s[n], want_kl[a][n], err_msg=f"KL sweep on A = {a}: {n}")
        np.testing.assert_array_equal(girsanov_level0_alt(plan, cqs[b], fb, prm), want_g[b], err_msg=f"Girsanov sweep on B = {b}")
    fa, fb = pair(plan, cqs[0], cqs[1])
    f2 = plan.cq_factor(cqs[2])                      # the first copy of the coarse levels now belongs to state 2
    s = plan.cq_selinv_kl(cqs[2], f2["L"], f2["y"], prm0, only_level=0)
    # (only_level = 0 after a plain factor: the coarse backward pass has not run -- the first copy's marginals are still A's, and
    #  using them must show; the full sweep then gives state 2's)
    assert not np.array_equal(host(s["klpart"]), want_kl[2]["klpart"])
    s = kl_host(amd, plan, plan.cq_selinv_kl(cqs[2], f2["L"], f2["y"], prm0))
    for n in ("x", "Sig", "klpart"):
        np.testing.assert_array_equal(s[n], want_kl[2][n], err_msg=f"KL sweep after a plain factor: {n}")
    np.testing.assert_array_equal(girsanov_level0_alt(plan, cqs[1], fb, prm), want_g[1], err_msg="Girsanov sweep on B after a plain factor")
    plan.check_info()


@pytest.mark.parametrize("d", [3, 6])
def test_pair_cache_policy(amd, d, monkeypatch):
    """MFGM_NT = 1, 2 (streamed stores: k_forward_pair_cq<D, 1>; 2 also streams the loads of the backward sweeps): only the load /
    store hint differs, so every result is bit-identical to MFGM_NT = 0."""
    case = PAIR_CASES[0]
    sd = np_cq.sde_inputs(d, "dw")

    def run(nt):
        monkeypatch.setenv("MFGM_NT", nt)
        refs, plan, cqs = states(amd, d, case, 2)
        st = refs[0]["st"]
        fa, fb = pair(plan, cqs[0], cqs[1])
        res = {"A " + n: v for n, v in owned(st, fa).items()}
        res.update({"B " + n: v for n, v in owned(st, fb).items()})
        s = kl_level0(amd, plan, cqs[0], st, fa, sde_params(amd, sd))
        res.update({"kl " + n: s[n] for n in ("x", "Sig", "klpart", "obs_mu", "obs_cov")})
        res["girsanov"] = girsanov_level0_alt(plan, cqs[1], fb, sde_params(amd, sd, LR))
        plan.check_info()
        return res

    base = run("0")
    for nt in ("1", "2"):
        got = run(nt)
        assert got.keys() == base.keys()
        for name in base:
            np.testing.assert_array_equal(got[name], base[name], err_msg=f"MFGM_NT={nt}: {name}")


@pytest.mark.parametrize("d", [3, 6, 8])
def test_pair_level_launches(amd, d):
    """A plan whose level 1 has 163 segments per chain (more than the 128 the fused coarse kernels take): that level runs as launches
    of its own, k_reduce_pair / k_forward_pair / k_backward_pair at double width.  Pair route against the single route, bit for bit."""
    shape = (2, 1300, 2, 4)
    sts = [np_cq.make_state(d, shape)]
    sts.append(np_cq.with_sites(sts[0], 1))
    st = sts[0]
    assert st.levels[1][2] > 128 and len(st.levels) >= 3
    plan = make_plan(amd, st)
    cqs = [device_state(amd, plan, s) for s in sts]
    cqs[1].dyn = cqs[0].dyn
    sd = np_cq.sde_inputs(d, "dw")
    prm0, prm = sde_params(amd, sd), sde_params(amd, sd, LR)
    # the single route: each sweep right after its own factorisation (the workspace holds the coarse levels of the latest one only)
    plain = [plan.cq_factor(cqs[0])]
    want_kl = plan.cq_selinv_kl(cqs[0], plain[0]["L"], plain[0]["y"], prm0)
    plain.append(plan.cq_factor(cqs[1]))
    want_g = sentinel_like(cqs[1].dyn)
    plan.cq_selinv_girsanov(cqs[1], plain[1]["L"], plain[1]["y"], prm, want_g)
    want_kl, want_g = kl_host(amd, plan, want_kl), host(want_g)
    fa, fb = pair(plan, cqs[0], cqs[1])
    same_factor(st, fa, plain[0], ("L", "y", "logdet"), "A")
    same_factor(st, fb, plain[1], ("L", "y"), "B")
    s = kl_host(amd, plan, plan.cq_selinv_kl(cqs[0], fa["L"], fa["y"], prm0, only_level=0))
    for n in ("x", "Sig", "klpart"):
        np.testing.assert_array_equal(s[n], want_kl[n], err_msg=n)
    np.testing.assert_array_equal(girsanov_level0_alt(plan, cqs[1], fb, prm), want_g)
    plan.check_info()


def test_cvi_dp_pair_steps_equal_unpipelined(amd, rng):
    """CVISitesSDE with the whole first factorisation of the next step made ahead (VIDP_PIPE_PAIR, Plan.cq_factor_pair) against the
    same model with the pipelining switched off, under the bound of test_cvi_dp_pipelined_steps_equal_unpipelined (1e-12): four loop
    steps on one pair of learning rates (records are consumed), the ELBO evaluated twice, another data learning rate (the record is
    refused), a snapshot, two steps, restore, the two steps again (the same numbers).  ELBOs, dyn, the sites and fx_*_obs are compared.
    (CVISitesSDE has no step_graph(); the batched trainer's replay is this snapshot / restore.)"""
    import torch
    from vidp_amd import sde as gsde
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.variational_cvi_sde import CVISitesSDE
    B, T, d, dt = 3, 1200, 3, 0.01
    grid = np.arange(T) * dt
    idx = np.arange(9, T - 1, 20)
    y = np.sign(rng.normal(size=(B, len(idx), d))) + 0.1 * rng.normal(size=(B, len(idx), d))
    cholR = 0.3 * np.eye(d)

    def make(pipe):
        m = CVISitesSDE(gsde.DoubleWellSDE(torch.eye(d, dtype=torch.float64)), grid, (grid[idx], dev(y)), MultivariateGaussian(dev(cholR)),
                        prior_initial_state=(np.zeros(d), np.eye(d)), plan=amd.Plan(B, T, d, R0=20, Rup=4))
        m.pipelined, m.pipe_pair, m.pipe_two_streams = pipe, True, False
        m.pipeline_min_nodes = 0
        return m
    a, b = make(False), make(True)
    assert b._cq_state() is not None
    alt_sweeps = []
    sweep = b.plan.cq_selinv_girsanov
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
    # steps 2-4, step 7 and the steps after the snapshot's and the restore's first one ran from a pair record; the first step, the one
    # after the change of the data learning rate and the one after restore factorised themselves
    # the first step and the one after the change of the data learning rate factorised themselves; every other one ran from a pair
    # record (the one after restore from the record the ELBO evaluated on the restored state made)
    assert alt_sweeps == [False, True, True, True, False, True, True, True, True, True], alt_sweeps
    assert b._ahead.consumed == sum(alt_sweeps)
    got, want = np.array(got), np.array(want)
    np.testing.assert_allclose(got, want, rtol=1e-12)
    np.testing.assert_array_equal(got[-3:], got[-6:-3])           # restore and the two steps after it repeat the snapshot's three
    for x, z, name in zip(state(b), state(a), ("dyn", "site_lin", "site_sym", "fx_mus_obs", "fx_covs_obs")):
        np.testing.assert_allclose(x, z, rtol=1e-12, atol=1e-12 * np.abs(z).max(), err_msg=name)
