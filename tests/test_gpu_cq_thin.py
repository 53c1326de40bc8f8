"""The thinned pair route: mfgm_cq_factor_pair_thin stores of the FIRST factor the records of the kept nodes only (even local steps
and step R - 1 of a level-0 segment), mfgm_cq_selinv_kl_thin rebuilds the others in registers; and CVISitesSDE on that route.

Kernels launched here: k_forward_pair_thin_cq<D, 0>, k_backward_kl_thin_cq<D, 0> (D = 1, 2, 3, 6), next to the full route's.

Shapes: every shape of np_cq_heads.SHAPES on the heads route (a one-node last segment, a ragged one, four tiles with padding lanes,
m = 1, an exact multiple), two with ODD segment lengths whose observed heads fall on rebuilt steps, and the plain route on the states
of np_cq.make_state, whose sites sit at arbitrary nodes (rebuilt ones among them).  The factor arrays are filled with NaN before a
thinned call: whatever the sweeps give is finite only if no record that was not stored is read.

Bounds: the kept records, logdet and the second factor equal the full route's bit for bit.  The sweeps are held to the 80-bit
reference of tests/np_cq.py under that module's rule max(8 x yardstick, 64 eps), the yardstick being the fp64 oracle's own error.
(The Girsanov sweep has no thinned form -- at d = 6 it would not fit the register file, DESIGN.md 5d -- so it runs on the full
second factor, through the second coarse copy.)"""
import ctypes
import functools

import numpy as np
import pytest

from tests import np_cq
from tests import np_cq_heads as nh
from tests import np_cq_thin as nt
from tests import test_gpu_cq as tq
from tests import test_gpu_cq_heads as th
from tests.test_gpu_cq import SENT, amd, check_marginals, dev, device_state, held, host, make_plan, sde_params, sentinel_like  # noqa: F401
from tests.test_gpu_cq_pair import LR, girsanov_level0_alt, sites

pytestmark = pytest.mark.gpu

DIMS = [1, 2, 3, 6]
ODD = [(3, 100, 9, 3, 3), (2, 47, 15, 3, 5)]
SHAPES = [("heads", s, i) for s, i in zip(nh.SHAPES, nh.SHAPE_IDS)] + [("heads", ODD[0], "B3-T100-R9-q3"), ("heads", ODD[1], "B2-T47-R15-q5")] + \
         [("plain", c, i) for c, i in zip(tq.CASES[:3], tq.CASE_IDS[:3])]
NEED_R = {ODD[0]: 9, ODD[1]: 15}
CASES = [(d, k, s) for k, s, _ in SHAPES for d in DIMS]
IDS = [f"{k}-{i}-d{d}" for k, _, i in SHAPES for d in DIMS]


def reference(kind, d, shape, nxt=0):
    """The cached references of the modules the states come from (computed once, shared with their tests)."""
    return th.reference(d, shape, nxt) if kind == "heads" else tq.reference(d, shape, nxt)


@functools.lru_cache(maxsize=None)
def reference_sweeps(kind, d, shape):
    """KL per chain of state 0 and dyn_out of the Girsanov sweep on state 1, each as (80-bit reference, fp64 oracle)."""
    sd = np_cq.sde_inputs(d, "dw")
    out = []
    for nxt in (0, 1):
        r = reference(kind, d, shape, nxt)
        args = (r["st"], sd.alpha, sd.beta, sd.qd, sd.dt, sd.init_mu, sd.init_cov)
        out.append(tuple(np_cq.kl_and_girsanov(*args, lr=[LR], post=r[k]) for k in ("ref", "orc")))
    return dict(kl=(out[0][0].kl, out[0][1].kl), dyn=(out[1][0].dyn_out[0], out[1][1].dyn_out[0]))


def states(amd, kind, d, shape, n=2):
    refs = [reference(kind, d, shape, k) for k in range(n)]
    st = refs[0]["st"]
    plan = make_plan(amd, st)
    stride = None
    if kind == "heads":
        stride = st.q
        assert plan.R % stride == 0
        if shape in NEED_R:
            assert plan.R == NEED_R[shape] and plan.R % 2 == 1
            keep = nt.kept_nodes(st.T, plan.R)
            assert np.any(~keep[st.obs_t]), "an observed head on a rebuilt step"
        else:
            assert plan.R == shape[2]
    elif plan.R > 2:                                     # (segments of two nodes: both are kept, the thinned route stores everything)
        assert np.any(~nt.kept_nodes(st.T, plan.R)[st.obs_t]), "a site on a rebuilt node"
    cqs = [device_state(amd, plan, r["st"]) for r in refs]
    for cq in cqs[1:]:
        cq.dyn = cqs[0].dyn
    return refs, plan, cqs, stride


def filled(plan, value):
    import torch
    return [dict(L=torch.full_like(plan.empty(3), value), y=torch.full_like(plan.empty(0), value)) for _ in range(2)]


def pair(plan, cqa, cqb, stride, thin, fill):
    out = filled(plan, fill)
    return plan.cq_factor_pair(cqa, sites(cqb), out=out[0], out2=out[1], head_stride=stride, thin=thin)


def kl_level0(amd, plan, cq, st, f, prm, want_marginals=True):
    """The level-0 KL sweep on the factor `f` (thinned or not, by its marker) into sentinel-filled outputs, in check_marginals' form."""
    import torch
    d, n_tot = st.d, st.obs_t.size
    obs_mu = torch.full((n_tot + 2, d), SENT, dtype=torch.float64, device="cuda")
    obs_cov = torch.full((n_tot + 2, d, d), SENT, dtype=torch.float64, device="cuda")
    out = dict(Sig=sentinel_like(plan.empty(amd.SYM)), x=sentinel_like(plan.empty(amd.VEC))) if want_marginals else None
    s = plan.cq_selinv_kl(cq, f["L"], f["y"], prm, out=out, obs_mu=obs_mu, obs_cov=obs_cov, only_level=0, want_marginals=want_marginals,
                          thin=f.get("thin", False))
    res = dict(klpart=host(s["klpart"]), obs_mu=host(obs_mu), obs_cov=host(obs_cov))
    if want_marginals:
        res.update(x=host(plan.unpack(amd.VEC, s["x"])), Sig=host(plan.unpack(amd.SYM, s["Sig"])), raw_x=host(s["x"]), raw_Sig=host(s["Sig"]))
    return res


def kept_flat(st, E, R):
    """Mask over a flat packed level-0 array with E doubles per node: the entries of kept nodes."""
    keep = np.broadcast_to(nt.kept_nodes(st.T, R)[None, :, None], (st.B, st.T, E)).astype(np.float64)
    fill = np.zeros(E)
    return np_cq.pack_nodes(np.ascontiguousarray(keep), st.levels[0], fill) == 1.0


@pytest.mark.parametrize("d,kind,shape", CASES, ids=IDS)
def test_thin_pair_records_and_sweeps(amd, d, kind, shape):
    """NaN guard, kept records, logdet, the KL sweep on A and the Girsanov sweep on B."""
    test = "thin_pair"
    refs, plan, cqs, stride = states(amd, kind, d, shape)
    st = refs[0]["st"]
    sd = np_cq.sde_inputs(d, "dw")
    full_a, full_b = pair(plan, cqs[0], cqs[1], stride, False, SENT)
    fa, fb = pair(plan, cqs[0], cqs[1], stride, True, float("nan"))
    assert fa["thin"] is True and not any("thin" in f for f in (fb, full_a, full_b))      # (no marker: a full factor)
    s = kl_level0(amd, plan, cqs[0], st, fa, sde_params(amd, sd))
    s_lazy = kl_level0(amd, plan, cqs[0], st, fa, sde_params(amd, sd), want_marginals=False)
    g = girsanov_level0_alt(plan, cqs[1], fb, sde_params(amd, sd, LR))
    plan.check_info()
    # kept records bit for bit; everything else of the thinned factor keeps its fill: never written
    for name, E in (("L", d * (d + 1) // 2), ("y", d)):
        got, want = host(fa[name]), host(full_a[name])
        keep = kept_flat(st, E, plan.R)
        own = np_cq.unpack_nodes(got, st.B, st.T, E, st.levels[0])[1]
        owned = own.sum()
        assert keep.shape == got.shape and keep.sum() == round(nt.stored_fraction(st.T, plan.R) * owned) and (keep.sum() < owned or plan.R == 2)
        np.testing.assert_array_equal(got[keep], want[keep], err_msg=f"kept records of {name}")
        assert not np.any(want[keep] == SENT)
        assert np.all(np.isnan(got[~keep])), f"{name}: a record that is not kept was written"
        np.testing.assert_array_equal(host(fb[name])[own], host(full_b[name])[own], err_msg=f"second factor {name}")
        assert np.all(np.isnan(host(fb[name])[~own]))
    np.testing.assert_array_equal(host(fa["logdet"]), host(full_a["logdet"]))
    # KL sweep on A: marginals everywhere and at the observations, KL per chain
    check_marginals(test, st, refs[0], fa, s)
    rs = reference_sweeps(kind, d, shape)
    held(test, "KL = kl_part + logdet - T d / 2", s["klpart"] + host(fa["logdet"]) - 0.5 * st.T * d, rs["kl"][0], rs["kl"][1])
    for name in ("klpart", "obs_mu", "obs_cov"):
        np.testing.assert_array_equal(s_lazy[name], s[name], err_msg=f"without the marginal arrays: {name}")
    # Girsanov sweep on B through the second coarse copy
    got, _ = np_cq.unpack_nodes(g, st.B, st.T, 3 * d, st.levels[0])
    assert not np.any(got == SENT)
    want, orc = rs["dyn"]
    T = st.T
    for name, sl, tt in (("lin", slice(0, d), T), ("diag", slice(d, 2 * d), T), ("sub", slice(2 * d, 3 * d), T - 1)):
        held(test, f"girsanov on B {name}", got[:, :tt, sl], want[:, :tt, sl], orc[:, :tt, sl])


@pytest.mark.parametrize("d,kind,shape", CASES, ids=IDS)
def test_thin_logdet_and_quad_equal_the_full_route(amd, d, kind, shape):
    """logdet AND quad of the thinned call, asked for through the entry itself (Plan.cq_factor_pair never asks for quad), against
    mfgm_cq_factor_pair / mfgm_cq_factor_pair_heads bit for bit; a staged thinned call writes neither."""
    import torch
    from vidp_amd.packed import _ptr, _stream
    refs, plan, cqs, stride = states(amd, kind, d, shape)
    a, b = cqs[0].struct(), cqs[0].struct()
    b.site_lin, b.site_sym = cqs[1].site_lin.data_ptr(), cqs[1].site_sym.data_ptr()
    scratch = plan._heads_scratch(stride) if stride else None
    n = scratch.numel() if stride else 0
    lib = plan.lib

    def call(which, stage=-1):
        arrs = [torch.full_like(plan.empty(k), float("nan")) for k in (3, 0, 3, 0)]
        sums = [torch.full((plan.B,), SENT, dtype=torch.float64, device="cuda") for _ in range(2)]
        head = (ctypes.byref(a), ctypes.byref(b), _ptr(arrs[0]), _ptr(arrs[1]), _ptr(sums[0]), _ptr(sums[1]), _ptr(arrs[2]), _ptr(arrs[3]))
        tail = (_ptr(plan.ws), _ptr(plan.info), _stream())
        if which == "thin":
            rc = lib.mfgm_cq_factor_pair_thin(plan.h, stage, stride or 0, *head, _ptr(scratch), n, *tail)
        elif stride:
            rc = lib.mfgm_cq_factor_pair_heads(plan.h, stride, *head, _ptr(scratch), n, *tail)
        else:
            rc = lib.mfgm_cq_factor_pair(plan.h, *head, *tail)
        assert rc == 0
        return [host(t) for t in sums]
    want, got = call("full"), call("thin")
    plan.check_info()
    for name, g, w in zip(("logdet", "quad"), got, want):
        assert np.all(np.isfinite(w)) and not np.any(w == SENT), name
        np.testing.assert_array_equal(g, w, err_msg=name)
    for stage in range(4):
        assert all(np.all(t == SENT) for t in call("thin", stage)), f"stage {stage} wrote logdet / quad"
    plan.check_info()


@pytest.mark.parametrize("d,kind,shape", CASES, ids=IDS)
def test_thin_calls_in_a_row_with_a_full_call_between(amd, d, kind, shape):
    """thin, full, thin into the SAME buffers: the marker follows the buffer's content and both thinned calls give the same numbers;
    the full call between them gives the full route's."""
    refs, plan, cqs, stride = states(amd, kind, d, shape)
    st = refs[0]["st"]
    prm = sde_params(amd, np_cq.sde_inputs(d, "dw"))
    out = filled(plan, float("nan"))
    res = []
    for thin in (True, False, True):
        fa, _ = plan.cq_factor_pair(cqs[0], sites(cqs[1]), out=out[0], out2=out[1], head_stride=stride, thin=thin)
        assert fa.get("thin", False) is thin and out[0]["thin"] is thin and out[1]["thin"] is False
        s = kl_level0(amd, plan, cqs[0], st, dict(L=out[0]["L"], y=out[0]["y"], thin=out[0]["thin"]), prm)
        res.append((s, host(fa["logdet"])))
    plan.check_info()
    want = pair(plan, cqs[0], cqs[1], stride, False, SENT)[0]
    ws = kl_level0(amd, plan, cqs[0], st, want, prm)
    for name in ("x", "Sig", "klpart", "obs_mu", "obs_cov"):
        np.testing.assert_array_equal(res[0][0][name], res[2][0][name], err_msg=f"thinned calls: {name}")
        np.testing.assert_array_equal(res[1][0][name], ws[name], err_msg=f"full call between: {name}")
        assert np.all(np.isfinite(res[0][0][name][res[0][0][name] != SENT]))
    for r in res:
        np.testing.assert_array_equal(r[1], host(want["logdet"]))


def test_thin_argument_errors(amd):
    """d > 6, a stage out of range, a stride the heads route refuses: reported, nothing launched."""
    import torch
    from vidp_amd.packed import _ptr, _stream
    refs, plan, cqs, _ = states(amd, "plain", 7, tq.CASES[1])
    with pytest.raises(ValueError, match="mfgm_cq_factor_pair_thin"):
        pair(plan, cqs[0], cqs[1], None, True, SENT)
    f = plan.cq_factor(cqs[0])
    prm = sde_params(amd, np_cq.sde_inputs(7, "dw"))
    with pytest.raises(ValueError, match="mfgm_cq_selinv_kl_thin"):
        plan.cq_selinv_kl(cqs[0], f["L"], f["y"], prm, thin=True)
    with pytest.raises(ValueError, match="mfgm_cq_selinv_kl_thin"):
        plan.cq_selinv_kl(cqs[0], f["L"], f["y"], prm, thin=True, only_level=0)
    with pytest.raises(ValueError, match="thinned"):
        plan.cq_selinv_girsanov(cqs[0], f["L"], f["y"], prm, torch.empty_like(cqs[0].dyn), thin=True)
    refs, plan, cqs, stride = states(amd, "heads", 3, nh.SHAPES[0])
    for bad in (-4, 1, 3, 5, 16):
        with pytest.raises(ValueError, match="mfgm_cq_factor_pair_thin"):
            pair(plan, cqs[0], cqs[1], bad, True, SENT)
    arrs = [sentinel_like(plan.empty(k)) for k in (3, 0, 3, 0)]
    a, b = cqs[0].struct(), cqs[0].struct()
    b.site_lin, b.site_sym = cqs[1].site_lin.data_ptr(), cqs[1].site_sym.data_ptr()
    for stage in (-2, 4):
        assert plan.lib.mfgm_cq_factor_pair_thin(plan.h, stage, 0, ctypes.byref(a), ctypes.byref(b), _ptr(arrs[0]), _ptr(arrs[1]), None, None,
                                                 _ptr(arrs[2]), _ptr(arrs[3]), None, 0, _ptr(plan.ws), _ptr(plan.info), _stream()) == 1
    torch.cuda.synchronize()
    assert all(bool((t == SENT).all()) for t in arrs)
    # a good call still works after the refused ones
    fa, _ = pair(plan, cqs[0], cqs[1], stride, True, float("nan"))
    plan.check_info()
    np.testing.assert_array_equal(host(fa["logdet"]), host(pair(plan, cqs[0], cqs[1], stride, False, SENT)[0]["logdet"]))


def test_cvi_dp_thin_factor_on_against_off(amd, rng):
    """CVISitesSDE, three steps at B = 3, T = 200, d = 2, segments of 40 nodes, an observation every 20: the thinned first factor
    (the default, VIDP_THIN_FACTOR) against the full one.  The sites are bit-identical; the ELBO and the marginals at the
    observations agree within 1e-12 of the largest entry (the bound of test_gpu_cq_heads for a reordered route); the marginal arrays
    asked for afterwards come from the thinned factor still in the buffers."""
    import torch
    from vidp_amd import sde as gsde
    from vidp_amd.likelihoods import MultivariateGaussian
    from vidp_amd.variational_cvi_sde import CVISitesSDE
    B, T, d, dt = 3, 200, 2, 0.01
    grid = np.arange(T) * dt
    idx = np.arange(20, T, 20)
    y = np.sign(rng.normal(size=(B, len(idx), d))) + 0.1 * rng.normal(size=(B, len(idx), d))
    cholR = 0.3 * np.eye(d)

    def make(thin):
        m = CVISitesSDE(gsde.DoubleWellSDE(torch.eye(d, dtype=torch.float64)), grid, (grid[idx], dev(y)), MultivariateGaussian(dev(cholR)),
                        prior_initial_state=(np.zeros(d), np.eye(d)), plan=amd.Plan(B, T, d, R0=40, Rup=4))
        m.pipelined, m.pipe_pair, m.pipe_two_streams, m.pair_heads, m.thin_factor = True, True, False, True, thin
        m.pipeline_min_nodes = 0
        assert m.plan.R == 40
        return m
    models = make(True), make(False)
    calls = {True: [], False: []}
    for m, thin in zip(models, (True, False)):
        fn, kl = m.plan.cq_factor_pair, m.plan.cq_selinv_kl
        m.plan.cq_factor_pair = lambda *a, _f=fn, _t=thin, **kw: (calls[_t].append(("pair", kw.get("thin"))), _f(*a, **kw))[1]
        m.plan.cq_selinv_kl = lambda *a, _f=kl, _t=thin, **kw: (calls[_t].append(("kl", kw.get("thin"))), _f(*a, **kw))[1]
    out = {True: [], False: []}
    for m, thin in zip(models, (True, False)):
        for _ in range(3):
            m.update_data_sites(0.5)
            m.update_girsanov_sites(0.1)
            out[thin].append(host(m.classic_elbo_per_trajectory()))
        m.plan.check_info()
        cq = m._cq_state()
        out[thin] += [host(t) for t in (m.fx_mus_obs, m.fx_covs_obs, m.data_nat1, cq.site_sym)]
        out[thin] += [np_cq.unpack_nodes(host(cq.dyn), B, T, 3 * d, np_cq.plan_levels(B, T, d, 40, 4)[0])[0]]      # (the records nodes own)
        out[thin] += [host(m.plan.unpack(amd.VEC, m._refresh(want_marginals=True)["mu"]))]
    assert ("pair", True) in calls[True] and ("kl", True) in calls[True] and calls[True][-1] == ("kl", True)
    assert all(t in (False, None) for _, t in calls[False])
    names = ["elbo 1", "elbo 2", "elbo 3", "fx_mus_obs", "fx_covs_obs", "site_lin", "site_sym", "dyn", "mu"]
    for name, got, want in zip(names, out[True], out[False]):
        if name in ("site_lin", "site_sym", "dyn"):
            np.testing.assert_array_equal(got, want, err_msg=name)
        else:
            err = np.abs(got - want).max() / np.abs(want).max()
            print(f"  {name}: thinned against full {err:.3e} of the largest entry")
            assert np.all(np.isfinite(got)) and err <= 1e-12, (name, err)
