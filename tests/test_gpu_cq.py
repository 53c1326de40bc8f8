"""
GPU tests of the structured-state ("cq") CVI-DP sweeps (csrc/mfgm_cq.h, the cq entry points of include/mfgm.h) against the 80-bit host
reference tests/np_cq.py, at every state dimension d = 1 ... 8, on every route of the dispatch in csrc/mfgm_api_sweeps.hip and at the
edges of the observation sites (node 0 where the site and p0_off meet, adjacent nodes, the ends of a segment, the separator, T - 1,
the padding-lane tile).  Inputs come from np_cq.make_state: nothing in them is negligibly small (d_off = -0.025, s_off = 0.03).

Tolerance rule.  Per output err = max |got - want| / max |want| against the 80-bit reference; the yardstick is the same figure for
the fp64 NumPy oracle on the same inputs, computed here; bound = max(8 x yardstick, 64 eps): a GPU result may be at most 8 x the
yardstick (the partitioned elimination sums in another order over up to three levels, each re-solving a separator system of similar
conditioning), with a floor of 64 eps for outputs the oracle happens to reproduce exactly.  On these inputs (condition number 3 - 5.5)
the yardstick is 0.1 ... 4 eps on nearly every output (tests/test_host_cq.py prints it), so 8 x yardstick is below the floor and
THE FLOOR IS WHAT BINDS: the effective bound is 64 eps.  Every check prints err, yardstick, err / yardstick and err / bound; a check
passes when err / bound <= 1.

Kernel instantiations and the test that launches them (D = 1 ... 8 unless noted):
  k_reduce_cq<D>, k_forward_cq<D, 0>, k_backward_kl_cq<D, 0>      test_cq_factor_and_kl_sweep
  k_mvn_ve_compact<D>, k_cq_elbo (mfgm_cq_elbo), k_sum_partials    test_cq_factor_and_kl_sweep
  k_backward_girsanov_cq<D, 0>, k_girsanov_fixup_cq<D>             test_cq_girsanov_sweep
  k_cq_pack<D>, k_cq_unpack<D>, k_cq_slots                         test_cq_equals_dense_entry_points (k_cq_slots: every test)
  k_forward_reduce_cq<D, 0> (D = 1 ... 6 only: it is not
  instantiated at D = 7, 8, nor is <D, 1>)                         test_cq_pipelined_forms, one stream
  k_reduce_cq_lean<D>                                              test_cq_pipelined_forms: side stream at every D; same stream at D = 7, 8
  k_forward_cq<D, 2>, k_backward_girsanov_cq<D, 2>,
  k_backward_kl_cq<D, 2>            D = 1, 3, 6, 8                 test_cq_cache_policy_variants (MFGM_NT=2)
  k_forward_reduce_cq<D, 1>         D = 1, 3, 6                    test_cq_cache_policy_variants (MFGM_NT=1 and 2)
  NOT launched by any test: the NT instantiations at D = 2, 4, 5, 7 (k_forward_cq<D, 2>, k_backward_*_cq<D, 2>; k_forward_reduce_cq<D, 1>
  at D = 2, 4, 5), and the coarse levels above level 0 are those of the dense route (held through every test here, not listed).

Largest err / bound measured on an MI355X, over every d, shape and output of a test (a test passes when <= 1), and the largest
err / yardstick behind it:
  test_cq_factor_and_kl_sweep     0.061  (obs_cov: err 8.6e-16, yardstick 5.5e-16)
  test_cq_girsanov_sweep          0.203 double well (lin, lr = 1: err 2.9e-15, yardstick 1.4e-15); 0.406 Ornstein-Uhlenbeck (lin at the
                                  separators, lr = 1: err 4.7e-14, yardstick 1.5e-14 of a near-zero output -- the one check where
                                  8 x yardstick, not the floor, is the bound); diag and sub 0.09
  test_cq_pipelined_forms         0.060  (Sig downstream of a from-record factor: err 8.6e-16, yardstick 5.2e-16)
  test_cq_cache_policy_variants   0.114  (dyn_out: err 1.6e-15, yardstick 6.9e-16)
Where the yardstick is at least 1 eps, err / yardstick was at most 6.4.

Checked once with two deliberately wrong scratch builds of the library (not committed): the sign of sOff flipped in cq_sub fails
test_cq_factor_and_kl_sweep at every d >= 2 (d = 1, which has no off-diagonal, passes); the p0off add dropped from
reduce_cq_lds_body fails the one-stream form of test_cq_pipelined_forms at every d = 2 ... 6 on the B3-T257 shape (at d = 1 p0_off
is empty, at d = 7, 8 and on a side stream that body is not run; on B1-T33 the 16-node first segment damps the change below 1e-12 at
d = 2, 4, 6).
"""
import functools

import numpy as np
import pytest

from tests import np_cq

pytestmark = pytest.mark.gpu

DIMS = list(range(1, 9))
FLOOR = 64 * np_cq.EPS
SENT = -7.0e77            # sentinel the outputs are pre-filled with
# (shape index, variant): the three shapes with sites and p0_off, one state without observation sites, one without p0_off
CASES = [(0, "full"), (1, "full"), (2, "full"), (1, "nosites"), (2, "nop0")]
CASE_IDS = ["B3-T257", "B1-T33", "B70-T9", "B1-T33-nosites", "B70-T9-nop0"]
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


# ---- references, computed once per (d, case) and shared ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(d, case, nxt=0):
    """State `nxt` of the case (0: the generator's, k > 0: the same with the k-th other set of data sites) with its 80-bit posterior and
    the fp64 oracle's."""
    si, variant = case
    st = np_cq.make_state(d, np_cq.SHAPES[si], sites=variant != "nosites", p0=variant != "nop0")
    if nxt:
        st = np_cq.with_sites(st, nxt)
    return dict(st=st, ref=np_cq.posterior(st), orc=np_cq.posterior_fp64(st))


@functools.lru_cache(maxsize=None)
def reference_kl(d, case, kind):
    r = reference(d, case)
    sd = np_cq.sde_inputs(d, kind)
    args = (r["st"], sd.alpha, sd.beta, sd.qd, sd.dt, sd.init_mu, sd.init_cov)
    lrs = [0.3, 1.0]
    return dict(sd=sd, lrs=lrs, ref=np_cq.kl_and_girsanov(*args, lr=lrs, post=r["ref"]), orc=np_cq.kl_and_girsanov(*args, lr=lrs, post=r["orc"]))


def held(test, name, got, want, oracle, scale=None):
    """The tolerance rule of the module docstring; prints err, yardstick and the two ratios.  scale: max |want| of the whole output
    when (got, want) is a subset of one."""
    err, yard = np_cq.rel_err(got, want, scale), np_cq.rel_err(oracle, want, scale)
    bound = max(8.0 * yard, FLOOR)
    WORST[test] = max(WORST.get(test, 0.0), err / bound)
    print(f"  {test} {name}: err {err:.3e}  yardstick {yard:.3e}  err / yardstick {err / yard if yard > 0 else float('inf'):.2f}  "
          f"err / bound {err / bound:.3f}  (largest err / bound so far in this test {WORST[test]:.3f})")
    assert np.all(np.isfinite(np.asarray(got, dtype=np.float64)))
    assert err <= bound, (name, err, yard)


# ---- device side ----------------------------------------------------------------------------------------------------------------------------
def make_plan(amd, st):
    B, T, R0, Rup = st.shape
    plan = amd.Plan(B, T, st.d, R0=R0, Rup=Rup)
    lv = st.levels[0]
    assert plan.nlevels == len(st.levels) >= 2 and (plan.R, plan.P, plan.Lpad) == (lv[1], lv[2], lv[3])
    return plan


def node_ids(st):
    return dev((np.arange(st.B)[:, None] * st.T + st.obs_t).reshape(-1).astype(np.int64))


def device_state(amd, plan, st):
    """CqState of a generated state; dyn and the slot array are laid out here (np_cq.pack_nodes, the layout of include/mfgm.h), the slot
    array of mfgm_cq_slots is held to the host one.  Records no node owns hold a harmless valid node, distinct from every live one."""
    from vidp_amd.packed import CqState
    d, lv = st.d, st.levels[0]
    fill = np.concatenate([np.zeros(d), np.full(d, -1.5), np.zeros(d)])
    dyn = dev(np_cq.pack_nodes(st.dyn, lv, fill))
    assert dyn.numel() == plan.lib.mfgm_cq_dyn_doubles(plan.h)
    cq = CqState(dyn, st.d_off, st.s_off, p0_off=None if st.p0_off is None else dev(np_cq.tril_pack(st.p0_off)))
    if st.obs_t is not None:
        slot = plan.cq_slots(node_ids(st))
        assert slot is not None and slot.numel() == plan.lib.mfgm_cq_slot_ints(plan.h)
        np.testing.assert_array_equal(host(slot), np_cq.slot_array(st, lv))
        cq.slot, cq.site_lin, cq.site_sym = slot, dev(st.site_lin), dev(np_cq.tril_pack(st.site_sym))
    return cq


def sde_params(amd, sd, lr=0.0):
    import torch
    from vidp_amd import sde as gsde
    q = torch.from_numpy(np.diag(sd.qd))
    gs = gsde.OrnsteinUhlenbeckSDE(sd.decay, q) if sd.kind == "ou" else gsde.DoubleWellSDE(q)
    prm = gs.params(sd.dt, sd.init_mu, sd.init_cov)
    assert prm.kind == 0
    prm.lr = float(lr)
    return prm


def owned(st, f):
    """Host copies of a factor dict; of the packed arrays L and y (made with torch.empty) only the entries a node owns."""
    d, out = st.d, {}
    for name, v in f.items():
        v = host(v)
        if name in ("L", "y"):
            v = np_cq.unpack_nodes(v, st.B, st.T, d if name == "y" else d * (d + 1) // 2, st.levels[0])[0]
        out[name] = v
    return out


def sentinel_like(t):
    import torch
    return torch.full_like(t, SENT)


def kl_sweep(amd, plan, cq, st, f, prm, want_marginals):
    """cq_selinv_kl into sentinel-filled outputs: dict(x, Sig natural or None, klpart, obs_mu, obs_cov with two spare rows, raw)."""
    import torch
    d = st.d
    n_tot = 0 if st.obs_t is None else st.obs_t.size
    obs_mu = torch.full((n_tot + 2, d), SENT, dtype=torch.float64, device="cuda")
    obs_cov = torch.full((n_tot + 2, d, d), SENT, dtype=torch.float64, device="cuda")
    out = dict(Sig=sentinel_like(plan.empty(amd.SYM)), x=sentinel_like(plan.empty(amd.VEC))) if want_marginals else None
    s = plan.cq_selinv_kl(cq, f["L"], f["y"], prm, out=out, obs_mu=obs_mu, obs_cov=obs_cov, want_marginals=want_marginals)
    plan.check_info()
    res = dict(klpart=host(s["klpart"]), obs_mu=host(obs_mu), obs_cov=host(obs_cov), x=None, Sig=None, t_mu=obs_mu, t_cov=obs_cov,
               t_kl=s["klpart"])
    if want_marginals:
        res.update(x=host(plan.unpack(amd.VEC, s["x"])), Sig=host(plan.unpack(amd.SYM, s["Sig"])), raw_x=host(s["x"]), raw_Sig=host(s["Sig"]))
    else:
        assert s["x"] is None and s["Sig"] is None
    return res


def check_marginals(test, st, r, f, s):
    """logdet, means, covariances and the observation-node copies against the reference; sentinels where nothing is to be written."""
    B, T, d = st.B, st.T, st.d
    ref, orc = r["ref"], r["orc"]
    if f.get("logdet") is not None:
        held(test, "logdet", host(f["logdet"]), ref.logdet, orc.logdet)
    held(test, "x", s["x"], ref.x, orc.x)
    held(test, "Sig", s["Sig"], ref.Sig, orc.Sig)
    np.testing.assert_array_equal(s["Sig"], np.swapaxes(s["Sig"], -1, -2))
    lv = st.levels[0]
    for raw, E in ((s["raw_x"], d), (s["raw_Sig"], d * (d + 1) // 2)):
        assert raw.size == lv[3] * lv[1] * E
        _, own = np_cq.unpack_nodes(raw, B, T, E, lv)
        assert np.all(raw[~own] == SENT) and not np.any(raw[own] == SENT)
    check_obs(test, st, r, s)


def check_obs(test, st, r, s):
    if st.obs_t is None:
        assert np.all(s["obs_mu"] == SENT) and np.all(s["obs_cov"] == SENT)
        return
    n_tot = st.obs_t.size
    ref, orc = r["ref"], r["orc"]
    held(test, "obs_mu", s["obs_mu"][:n_tot].reshape(st.B, -1, st.d), np_cq.at_obs(st, ref.x), np_cq.at_obs(st, orc.x))
    held(test, "obs_cov", s["obs_cov"][:n_tot].reshape(st.B, -1, st.d, st.d), np_cq.at_obs(st, ref.Sig), np_cq.at_obs(st, orc.Sig))
    assert np.all(s["obs_mu"][n_tot:] == SENT) and np.all(s["obs_cov"][n_tot:] == SENT)


# ---- the tests ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dw", "ou"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("d", DIMS)
def test_cq_factor_and_kl_sweep(amd, d, case, kind):
    """mfgm_cq_factor + mfgm_cq_selinv_kl (k_reduce_cq, k_forward_cq, k_backward_kl_cq and the coarse levels), mfgm_mvn_ve_compact and
    mfgm_cq_elbo against the 80-bit reference; without the marginal arrays the sweep gives the same sums and observation-node marginals
    bit for bit."""
    test = "factor_and_kl"
    r, k = reference(d, case), reference_kl(d, case, kind)
    st = r["st"]
    B, T = st.B, st.T
    plan = make_plan(amd, st)
    cq = device_state(amd, plan, st)
    prm = sde_params(amd, k["sd"])
    f = plan.cq_factor(cq)
    s = kl_sweep(amd, plan, cq, st, f, prm, True)
    check_marginals(test, st, r, f, s)
    logdet = host(f["logdet"])
    held(test, "KL = kl_part + logdet - T d / 2", s["klpart"] + logdet - 0.5 * T * d, k["ref"].kl, k["orc"].kl)
    # the marginal arrays left out: the same arithmetic with the stores skipped
    s2 = kl_sweep(amd, plan, cq, st, f, prm, False)
    for name in ("klpart", "obs_mu", "obs_cov"):
        np.testing.assert_array_equal(s2[name], s[name], err_msg=name)
    if st.obs_t is None:
        return
    # variational expectations and the ELBO from what the sweeps left on the device
    import math
    from oracle import np_models
    n = st.obs_t.shape[1]
    Sinv = np_cq.spd_inverse(st.cholR @ st.cholR.T).astype(np.float64)
    cst = -float(np.sum(np.log(np.diag(st.cholR)))) - 0.5 * d * math.log(2.0 * math.pi)
    ve_part = plan.mvn_ve_compact(s2["t_mu"], s2["t_cov"], n, dev(st.y.reshape(B * n, d)), dev(Sinv), cst, partials=True)
    assert tuple(ve_part.shape) == (B, 1)
    elbo, total = plan.cq_elbo(ve_part, s2["t_kl"], f["logdet"], -0.5 * T * d)
    ref, orc = r["ref"], r["orc"]
    ve_ref = np_cq.ve_compact(np_cq.at_obs(st, ref.x), np_cq.at_obs(st, ref.Sig), st.y, st.cholR)
    ve_orc = np_models.MultivariateGaussianLik(st.cholR).variational_expectations(np_cq.at_obs(st, orc.x), np_cq.at_obs(st, orc.Sig), st.y).sum(-1)
    held(test, "ve", host(ve_part).sum(-1), ve_ref, ve_orc)
    e_ref, tot_ref = np_cq.elbo(ve_ref, k["ref"].kl)
    e_orc, tot_orc = np_cq.elbo(ve_orc, k["orc"].kl)
    held(test, "elbo", host(elbo), e_ref, e_orc)
    # the total: one number; its error and its yardstick are both normalised by the sum of the magnitudes it adds up
    held(test, "elbo total", host(total), tot_ref, tot_orc, scale=np.abs(e_ref).sum())


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("d", DIMS)
def test_cq_girsanov_sweep(amd, d, case):
    """mfgm_cq_selinv_girsanov (k_backward_girsanov_cq + k_girsanov_fixup_cq) against (1 - lr) dyn + lr (theta_q - grad KL) of the
    reference, at lr = 0.3 and 1; the separator nodes (the last node of every segment, whose linear part the fix-up kernel completes)
    are checked on their own."""
    r = reference(d, case)
    st = r["st"]
    B, T = st.B, st.T
    n, R, P, _ = st.levels[0]
    plan = make_plan(amd, st)
    cq = device_state(amd, plan, st)
    f = plan.cq_factor(cq, want_logdet=False)
    sep = np.minimum(np.arange(1, P + 1) * R, T) - 1
    # (the separator subsets are normalised by the largest entry of the whole output: under the Ornstein-Uhlenbeck drift theta~_lin
    #  vanishes away from node 0, and at lr = 1 a subset without node 0 has nothing but rounding to be normalised by)
    for kind, lr, want, orc in [(kind, *z) for kind in ("dw", "ou") for k in [reference_kl(d, case, kind)]
                                for z in zip(k["lrs"], k["ref"].dyn_out, k["orc"].dyn_out)]:
        k, test = reference_kl(d, case, kind), "girsanov " + kind
        out = sentinel_like(cq.dyn)
        plan.cq_selinv_girsanov(cq, f["L"], f["y"], sde_params(amd, k["sd"], lr), out)
        plan.check_info()
        got, _ = np_cq.unpack_nodes(host(out), B, T, 3 * d, st.levels[0])
        assert not np.any(got == SENT)
        for name, sl, tt in (("lin", slice(0, d), T), ("diag", slice(d, 2 * d), T), ("sub", slice(2 * d, 3 * d), T - 1)):
            held(test, f"lr={lr} {name}", got[:, :tt, sl], want[:, :tt, sl], orc[:, :tt, sl])
            ts = sep[sep < tt]
            held(test, f"lr={lr} {name} at the separators", got[:, ts, sl], want[:, ts, sl], orc[:, ts, sl],
                 scale=np.abs(want[:, :tt, sl]).max())
        # the last node has no transition: its diag-of-sub entry is carried over as it is
        np.testing.assert_array_equal(got[:, T - 1, 2 * d:], st.dyn[:, T - 1, 2 * d:])


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("d", DIMS)
def test_cq_equals_dense_entry_points(amd, d, case):
    """The cq sweeps against the dense entry points (mfgm_packed_factor with scales (-2, -1, 1), mfgm_packed_selinv_kl,
    mfgm_packed_selinv_girsanov) on the naturals mfgm_cq_unpack + the scattered sites give; mfgm_cq_pack inverts mfgm_cq_unpack;
    mfgm_cq_slots reports a repeated node."""
    import torch
    r = reference(d, case)
    st = r["st"]
    B, T = st.B, st.T
    sd = np_cq.sde_inputs(d, "dw")
    prm = sde_params(amd, sd, 0.3)
    plan = make_plan(amd, st)
    cq = device_state(amd, plan, st)
    f = plan.cq_factor(cq)
    s = kl_sweep(amd, plan, cq, st, f, prm, True)
    logdet = host(f["logdet"])
    dyn_out = sentinel_like(cq.dyn)
    plan.cq_selinv_girsanov(cq, f["L"], f["y"], prm, dyn_out)
    g, _ = np_cq.unpack_nodes(host(dyn_out), B, T, 3 * d, st.levels[0])

    # unpack: exactly the dense naturals without the sites (fp64 sums of the same terms)
    lin, diag, sub = plan.cq_unpack(cq)
    eye = np.eye(d)
    want_diag = st.dyn[..., d:2 * d, None] * eye + st.d_off * (1 - eye)
    if st.p0_off is not None:
        want_diag[:, 0] = want_diag[:, 0] + st.p0_off
    want_sub = st.dyn[:, :T - 1, 2 * d:, None] * eye + st.s_off * (1 - eye)
    np.testing.assert_array_equal(host(plan.unpack(amd.VEC, lin)), st.dyn[..., :d])
    np.testing.assert_array_equal(host(plan.unpack(amd.SYM, diag)), want_diag)
    np.testing.assert_array_equal(host(plan.unpack(amd.FULL, sub, T - 1)), want_sub)
    # pack(unpack): dyn exactly (the entry that stands for no transition becomes 0), the off-diagonal ranges collapsed on d_off, s_off
    dyn2, (dlo, dhi), (slo, shi) = plan.cq_pack(lin, diag, sub)
    back, _ = np_cq.unpack_nodes(host(dyn2), B, T, 3 * d, st.levels[0])
    want_dyn = st.dyn.copy()
    want_dyn[:, T - 1, 2 * d:] = 0.0
    np.testing.assert_array_equal(back, want_dyn)
    if d > 1:
        assert (dlo, dhi, slo, shi) == (st.d_off, st.d_off, st.s_off, st.s_off)

    # the dense route on the same naturals
    if st.obs_t is not None:
        ids = node_ids(st)
        plan.scatter_nodes(amd.VEC, lin, ids, dev(st.site_lin), accumulate=True)
        plan.scatter_nodes(amd.SYM, diag, ids, dev(np.broadcast_to(st.site_sym, (ids.numel(), d, d))), accumulate=True)
        # a node observed twice cannot be represented
        assert plan.cq_slots(torch.cat([ids, ids[3:4]])) is None
        assert plan.cq_slots(ids) is not None
    fd = plan.factor(diag, sub, lin, aD=-2.0, aS=-1.0, aR=1.0, store_G=False)
    kd = plan.selinv_kl(fd["L"], sub, -1.0, fd["y"], prm)
    out = (plan.zeros(amd.VEC), plan.zeros(amd.SYM), plan.zeros(amd.FULL))
    plan.selinv_girsanov(fd["L"], sub, -1.0, fd["y"], prm, (lin, diag, sub), out)
    plan.check_info()

    def same(a, b, name):
        np.testing.assert_allclose(a, b, rtol=1e-10, atol=1e-11 * max(1.0, np.abs(b).max()), err_msg=name)
    same(logdet, host(fd["logdet"]), "logdet")
    same(s["x"], host(plan.unpack(amd.VEC, kd["x"])), "x")
    same(s["Sig"], host(plan.unpack(amd.SYM, kd["Sig"])), "Sig")
    same(s["klpart"], host(kd["klpart"]), "klpart")
    o1, od, os_ = host(plan.unpack(amd.VEC, out[0])), host(plan.unpack(amd.SYM, out[1])), host(plan.unpack(amd.FULL, out[2], T - 1))
    if st.obs_t is not None:
        # the dense sweep writes (1 - lr) theta_q + lr theta~ with the sites in theta_q; the cq state holds theta_q without them
        bi, ti = np.repeat(np.arange(B), st.obs_t.shape[1]), st.obs_t.reshape(-1)
        np.subtract.at(o1, (bi, ti), (1.0 - prm.lr) * st.site_lin)
        np.subtract.at(od, (bi, ti), np.broadcast_to((1.0 - prm.lr) * st.site_sym, (len(bi), d, d)))
    same(g[..., :d], o1, "girsanov lin")
    same(g[..., d:2 * d], np.diagonal(od, axis1=-2, axis2=-1), "girsanov diag")
    same(g[:, :T - 1, 2 * d:], np.diagonal(os_, axis1=-2, axis2=-1), "girsanov sub")


def _ulps(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float((np.abs(a - b) / np.maximum(np.spacing(np.abs(b)), np.finfo(np.float64).tiny)).max())


@pytest.mark.parametrize("streams", [False, True], ids=["one-stream", "side-stream"])
@pytest.mark.parametrize("case", CASES[:3], ids=CASE_IDS[:3])
@pytest.mark.parametrize("d", DIMS)
def test_cq_pipelined_forms(amd, d, case, streams):
    """mfgm_cq_factor_pipelined in every form of cq_factor_impl: without a side stream the two-wavefront LDS kernel k_forward_reduce_cq
    (d <= 6) or k_forward_cq followed by k_reduce_cq_lean on the same stream (d = 7, 8); with one, k_reduce_cq_lean on the side stream.
    Two pipelined calls in a row (the two level-1 regions swap roles twice), then the factorisation from the last record.  The factor
    made alongside equals plain mfgm_cq_factor on the current state, the one made from a record plain mfgm_cq_factor on the state the
    record was made for (1e-12; measured on an MI355X: bit-identical with k_reduce_cq_lean, which is asserted, and within 2.5e-16 of
    the largest entry with the LDS body of k_forward_reduce_cq, which orders the sums of rho differently: d = 2 ... 6, up to 192 ulp
    of a small entry), and the marginals downstream of a from-record factor are held to the reference."""
    import torch
    test = "pipelined"
    refs = [reference(d, case, k) for k in range(3)]
    sts = [r["st"] for r in refs]
    plan = make_plan(amd, sts[0])
    cqs = [device_state(amd, plan, st) for st in sts]
    cqs[1].dyn = cqs[2].dyn = cqs[0].dyn              # one resident state, three sets of data sites
    prm = sde_params(amd, np_cq.sde_inputs(d, "dw"))
    keep = lambda f: owned(sts[0], f)
    plain = [keep(plan.cq_factor(cq)) for cq in cqs]
    side = torch.cuda.Stream() if streams else None
    sites = lambda cq: (cq.site_lin, cq.site_sym)
    got, sweeps = [], []
    for i in range(3):
        f = plan.cq_factor(cqs[i], use_ahead=i > 0, next_sites=sites(cqs[i + 1]) if i < 2 else None, side=side)
        got.append(keep(f))
        sweeps.append(kl_sweep(amd, plan, cqs[i], sts[i], f, prm, True) if i > 0 else None)
    torch.cuda.synchronize()
    plan.check_info()
    worst = 0.0
    for i in range(3):
        for name in ("L", "y", "logdet"):
            a, b = got[i][name], plain[i][name]
            u = _ulps(a, b)
            worst = max(worst, u)
            print(f"  {test} step {i} {name}: largest difference from mfgm_cq_factor {u:.1f} ulp, relative "
                  f"{np.abs(a - b).max() / np.abs(b).max():.3e}")
            assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), (i, name)
            if streams or d > 6:                     # k_reduce_cq_lean is k_reduce_cq's body with its accumulators in LDS
                np.testing.assert_array_equal(a, b, err_msg=f"step {i} {name}")
    print(f"  {test} d={d} {case} streams={streams}: largest difference {worst:.1f} ulp")
    for i in (1, 2):
        check_marginals(test, sts[i], refs[i], dict(logdet=None), sweeps[i])


@pytest.mark.parametrize("d", [1, 3, 6, 8])
def test_cq_cache_policy_variants(amd, d, monkeypatch):
    """The cache-policy instantiations (MFGM_NT = 1: streamed stores, k_forward_reduce_cq<D, 1>; 2: also streamed loads, k_forward_cq<D, 2>,
    k_backward_girsanov_cq<D, 2>, k_backward_kl_cq<D, 2>), which the library picks for arrays of 128 MB and more, on the first shape:
    only the load / store hint differs, so every result is bit-identical to MFGM_NT = 0; and within the reference bound."""
    import torch
    test = "cache_policy"
    case = CASES[0]
    refs = [reference(d, case, k) for k in range(2)]
    k = reference_kl(d, case, "dw")
    st = refs[0]["st"]

    def run(nt):
        monkeypatch.setenv("MFGM_NT", nt)
        plan = make_plan(amd, st)
        cqs = [device_state(amd, plan, r["st"]) for r in refs]
        cqs[1].dyn = cqs[0].dyn
        prm = sde_params(amd, k["sd"], 0.3)
        res = {}
        f = plan.cq_factor(cqs[0])
        res.update({"factor " + n: v for n, v in owned(st, f).items()})
        s = kl_sweep(amd, plan, cqs[0], st, f, prm, True)
        s2 = kl_sweep(amd, plan, cqs[0], st, f, prm, False)
        out = sentinel_like(cqs[0].dyn)
        plan.cq_selinv_girsanov(cqs[0], f["L"], f["y"], prm, out)
        res.update({"kl " + n: s[n] for n in ("x", "Sig", "klpart", "obs_mu", "obs_cov")})
        res.update({"lazy " + n: s2[n] for n in ("klpart", "obs_mu", "obs_cov")})
        res["girsanov"] = host(out)
        for tag, side in (("one-stream", None), ("side-stream", torch.cuda.Stream())):
            f1 = plan.cq_factor(cqs[0], next_sites=(cqs[1].site_lin, cqs[1].site_sym), side=side)
            f2 = plan.cq_factor(cqs[1], use_ahead=True, side=side)
            s3 = kl_sweep(amd, plan, cqs[1], refs[1]["st"], f2, prm, True)
            torch.cuda.synchronize()
            res.update({f"{tag} alongside {n}": v for n, v in owned(st, f1).items()})
            res.update({f"{tag} from record {n}": v for n, v in owned(st, f2).items()})
            res.update({f"{tag} from record {n}": s3[n] for n in ("x", "Sig", "klpart")})
        plan.check_info()
        return res, dict(f=f, s=s)

    base, _ = run("0")
    for nt in ("1", "2"):
        got, h = run(nt)
        assert got.keys() == base.keys()
        for name in base:
            np.testing.assert_array_equal(got[name], base[name], err_msg=f"MFGM_NT={nt}: {name}")
        check_marginals(test, st, refs[0], h["f"], h["s"])
        held(test, "KL", h["s"]["klpart"] + host(h["f"]["logdet"]) - 0.5 * st.T * d, k["ref"].kl, k["orc"].kl)
        g, _ = np_cq.unpack_nodes(got["girsanov"], st.B, st.T, 3 * d, st.levels[0])
        held(test, "girsanov", g[:, :st.T - 1], k["ref"].dyn_out[0][:, :st.T - 1], k["orc"].dyn_out[0][:, :st.T - 1])
