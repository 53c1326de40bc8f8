"""
GPU tests of mini-batch sparse CVI: k_sparse_batch / k_batch_seg (csrc/mfgm_minibatch.h; entry points
mfgm_sparse_batch_predict_lik, mfgm_sparse_batch_seg) through the C ABI against the np.longdouble restatement tests/np_minibatch.py on
identical inputs for every block size, SparseCVIGaussianProcess(num_data=) against the restatement, against the full-batch route and
against its own torch route, what is out of scope, and MiniBatchSitesTrainer.  fp64.

Every test here fails on a tree without the feature: the symbols, the keyword and the trainer do not exist there.

Measured on an MI355X: kernel against long double w 8.9e-16, c 1.0e-15 of max(1, max |row|) and fmu 9.2e-16, fvar 9.0e-16, ve 4.2e-15,
g1 1.7e-15, g2 4.2e-15, ve_sum 8.7e-16 of the absolute sums (bounds 1e-12); one epoch against the full batch 5.4e-16 (1e-12); steps
against the restatement: bound 6.3e-16 (1e-9), sites 6.8e-16 (1e-10), the d = 9 Sum on the torch route 2.1e-15; a whole batch
against the full-batch route 8.4e-16 (1e-12); torch route against native 1.8e-15 (5e-12).
"""
import ctypes

import numpy as np
import pytest

from tests import np_hyper as H
from tests import np_minibatch as MB
from tests import np_sparse_hyper as S
from tests.test_gpu_sparse_hyper import KERNEL_CASES, M_K, SUM9, TREES, _kernel_times, _pair_chain

pytestmark = pytest.mark.gpu

ROW_TOL = 1e-12           # w, c: of max(1, max |row|) -- the project's bound for its register-resident closed-form kernels
SUM_TOL = 1e-12           # fmu, fvar, ve, g1, g2, ve_sum: of the sum of the absolute terms of the quantity
ELBO_TOL, SITE_TOL = 1e-9, 1e-10
FULL_TOL = 1e-12          # a whole shuffled batch against the sorted full-batch route; one epoch against the full batch
ROUTE_TOL = 5e-12         # torch route against native, as test_gpu_sparse_hyper.test_torch_route_equals_native
LIKS = {"gaussian": ("gaussian", 0.3), "bernoulli": ("bernoulli", 1e-3), "poisson": ("poisson", 0.7)}
KIND = {"gaussian": 3, "bernoulli": 1, "poisson": 2}
OUTS = ["idx", "w", "c", "fmu", "fvar", "ve", "g1", "g2", "ve_sum"]


@pytest.fixture(scope="module")
def amd():
    import torch
    import vidp_amd
    assert torch.cuda.is_available()
    vidp_amd._lib.load()
    return vidp_amd


def dev(x, dtype=np.float64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def host(x):
    return x.detach().cpu().numpy()


def rel(got, ref):
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))


def of_largest(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


# ---- 1. the kernel alone ------------------------------------------------------------------------------------------------------------------
def batch_call(amd, kt, d, z, t, moments, pm, P0, kind=0, param=0.0, scale=1.0, y=None, shift=None, skip=()):
    """One call of mfgm_sparse_batch_predict_lik on sentinel-filled outputs; the outputs named in `skip` (and the likelihood's with
    kind 0) are passed as NULL.  Returns (dict of the output tensors, info)."""
    import torch
    lib = amd._lib.load()
    n = int(t.shape[0])
    f = lambda *shape: torch.full(shape, 7.0, dtype=torch.float64, device="cuda")
    out = dict(idx=torch.full((n,), -7, dtype=torch.int32, device="cuda"), w=f(n, 2 * d), c=f(n), fmu=f(n), fvar=f(n), ve=f(n), g1=f(n),
               g2=f(n), ve_sum=f(1))
    none = set(skip) | ({"ve", "g1", "g2", "ve_sum"} if kind == 0 else set())
    nws = int(lib.mfgm_sparse_batch_workspace_doubles(n))
    ws = f(nws + 4)
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    ptr = lambda x: None if x is None else x.data_ptr()
    rc = lib.mfgm_sparse_batch_predict_lik(ctypes.byref(kt), int(z.shape[0]), z.data_ptr(), n, t.data_ptr(), ptr(shift), kind, param, scale,
                                           ptr(y), pm.data_ptr(), P0.data_ptr(), *[m.data_ptr() for m in moments],
                                           *[None if k in none else out[k].data_ptr() for k in OUTS], ws.data_ptr(), info.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((ws[nws:] == 7.0).all())          # nothing past the workspace the size function asked for
    for k in none:
        assert bool((out[k] == (-7 if k == "idx" else 7.0)).all()), f"{k} was passed as NULL and written"
    return out, int(info.item())


def _batch_times(rng, spec, n):
    """Inducing points and n time points in any order: those of test_gpu_sparse_hyper._kernel_times (both end intervals populated,
    interval 2 empty, two points at one time, one point exactly on an inducing point) plus, for n > 1, one non-finite time; shuffled."""
    if n == 1:
        return _kernel_times(rng, spec, 1)
    z, t = _kernel_times(rng, spec, n - 1)
    t = np.concatenate([t, [np.nan if n == 70 else np.inf]])
    return z, t[rng.permutation(n)]


@pytest.mark.parametrize("n", [1, 70, 130])
@pytest.mark.parametrize("tree,jitter", KERNEL_CASES, ids=[f"{t}-{j:g}" for t, j in KERNEL_CASES])
def test_batch_kernel_against_long_double(amd, rng, tree, jitter, n):
    """mfgm_sparse_batch_predict_lik through the C ABI against the np.longdouble restatement on identical inputs: M = 5, n = 1, 70 (a
    partial wavefront next to a full one) and 130 (three wavefronts: the cross-wavefront order of ve_sum), unsorted times, random
    positive definite pair moments and a non-zero prior mean; the cases with a jitter also carry a shift and scale = 3.7.
    idx exactly; w, c within 1e-12 of max(1, max |row|); fmu, fvar, ve, g1, g2, ve_sum within 1e-12 of the sum of the absolute terms of
    the quantity, for kind 0 and the three likelihoods; exact zeros for NaN observations and the non-finite time; identical bits on a
    second call; info == 0; outputs passed as NULL untouched.
    Measured values: the head of this file and DESIGN.md section 26."""
    import torch
    spec = TREES[tree][0]
    d = H.state_dim(spec)
    z, t = _batch_times(rng, spec, n)
    fin = np.isfinite(t)
    if n > 1:
        idx, glo, ghi = S.gaps(t[fin], z)
        assert (idx == 0).sum() >= 2 and (idx == M_K).sum() >= 2 and (idx == 2).sum() == 0 and (ghi == 0.0).sum() == 1
        assert (np.diff(np.sort(t[fin])) == 0.0).sum() == 1 and (~fin).sum() == 1 and (np.diff(t[fin]) < 0).any()
    mu, Sig, Sub = _pair_chain(rng, M_K, d)
    pm = 0.3 * rng.normal(size=d)
    P0 = S.transition(spec, jitter, 0.0, np.float64)[2] + jitter * np.eye(d)
    shifted = jitter != 0.0
    shift = rng.normal(size=n) if shifted else None
    scale = 3.7 if shifted else 1.0
    f = 0.5 * rng.normal(size=n)
    ys = dict(gaussian=f + 0.3 * rng.normal(size=n), bernoulli=(f > 0).astype(np.float64), poisson=rng.poisson(np.exp(f)).astype(np.float64))
    absent = rng.choice(n, 3, replace=False) if n > 1 else np.zeros(0, dtype=np.int64)
    for y in ys.values():
        y[absent] = np.nan
    kt = H.build_vidp(spec, jitter)._terms_struct()
    args = dict(z=dev(z), t=dev(t), moments=[dev(mu), dev(Sig), dev(Sub)], pm=dev(pm), P0=dev(P0), shift=None if shift is None else dev(shift))
    worst = {}

    def check(name, got, ref, sc):
        assert np.isfinite(got).all(), f"{name} is not finite"
        e = np.abs(got - np.asarray(ref, dtype=np.float64)) / np.maximum(np.asarray(sc, dtype=np.float64), 1e-300)
        worst[name] = max(worst.get(name, 0.0), float(np.max(e)))

    for lik in [None, "gaussian", "bernoulli", "poisson"]:
        kw = dict(args) if lik is None else dict(args, kind=KIND[lik], param=LIKS[lik][1], scale=scale, y=dev(ys[lik]))
        out, info = batch_call(amd, kt, d, **kw)
        again, _ = batch_call(amd, kt, d, **kw)
        assert info == 0
        for k in OUTS:
            assert torch.equal(out[k], again[k]), f"{k}: two calls differ"
        ref = MB.batch_pass(spec, jitter, z, t, mu, Sig, Sub, pm, P0, None if lik is None else LIKS[lik], None if lik is None else ys[lik],
                            scale, shift)
        g = {k: host(v) for k, v in out.items()}
        assert np.array_equal(g["idx"], ref["idx"])
        row_scale = np.maximum(1.0, np.maximum(np.abs(ref["w"]).max(1), np.abs(ref["c"]))).astype(np.float64)
        check("w", g["w"], ref["w"], row_scale[:, None])
        check("c", g["c"], ref["c"], row_scale)
        for k in ("fmu", "fvar") + (() if lik is None else ("ve", "g1", "g2", "ve_sum")):
            check(k, g[k], ref[k], ref["scale"][k])
        # exact zeros
        assert (g["w"][~fin] == 0).all() and (g["c"][~fin] == 0).all() and (g["fvar"][~fin] == 0).all()
        assert (g["fmu"][~fin] == (0.0 if shift is None else shift[~fin])).all()
        if lik is not None:
            off = ~fin
            off[absent] = True
            for k in ("ve", "g1", "g2"):
                assert (g[k][off] == 0).all() and (g[k][~off] != 0).all()
            assert np.isfinite(g["fmu"]).all() and (g["fvar"][fin] > 0).all()
    print(f"{tree} jitter {jitter} n {n}: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert max(worst["w"], worst["c"]) <= ROW_TOL
    assert max(v for k, v in worst.items() if k not in ("w", "c")) <= SUM_TOL
    # a subset of the outputs alone: the same bits, the others untouched (checked in batch_call)
    lik = "poisson"
    kw = dict(args, kind=KIND[lik], param=LIKS[lik][1], scale=scale, y=dev(ys[lik]))
    full, _ = batch_call(amd, kt, d, **kw)
    part, _ = batch_call(amd, kt, d, skip=("idx", "w", "fvar", "g1", "ve"), **kw)
    for k in ("c", "fmu", "g2", "ve_sum"):
        assert torch.equal(part[k], full[k])
    part, _ = batch_call(amd, kt, d, skip=("c", "fmu", "g2", "ve_sum"), **kw)
    for k in ("idx", "w", "fvar", "g1", "ve"):
        assert torch.equal(part[k], full[k])


def test_batch_kernel_reports_a_q_that_is_not_positive_definite(amd, rng):
    """A Constant term has no process noise: with a NEGATIVE jitter its Q_mp block is neither positive definite nor zero and *info is
    set (no fault: the lane's row is NaN); the same tree with jitter 1e-6 leaves it at 0 (test above)."""
    spec = TREES["sum_prod_m12_h_const"][0]
    d = H.state_dim(spec)
    z, t = _batch_times(rng, spec, 70)
    mu, Sig, Sub = _pair_chain(rng, M_K, d)
    kt = H.build_vidp(spec, 1e-6)._terms_struct()
    kt.jitter = -1e-3
    _, info = batch_call(amd, kt, d, dev(z), dev(t), [dev(mu), dev(Sig), dev(Sub)], dev(np.zeros(d)), dev(np.eye(d)))
    assert info != 0


# ---- 2. the CSR offsets ---------------------------------------------------------------------------------------------------------------------
def test_batch_seg_against_searchsorted(amd, rng):
    """mfgm_sparse_batch_seg equals the np.searchsorted-derived offsets exactly: the sorted times of test 1 (ties, a point on an inducing
    point, an empty interval, NaN last), n = 0, and batches that lie entirely in one end interval; M + 2 beyond one wavefront too."""
    import torch
    lib = amd._lib.load()
    spec = TREES["matern32"][0]
    z5, t = _batch_times(rng, spec, 130)
    z100 = np.cumsum(rng.uniform(0.5, 1.5, 100))
    cases = [(z5, np.sort(t)), (z5, np.zeros(0)), (z5, z5[0] - 1.0 - rng.uniform(size=9).cumsum()[::-1]), (z5, z5[-1] + rng.uniform(size=9).cumsum()),
             (z100, np.sort(rng.uniform(-3.0, z100[-1] + 3.0, 333))), (z100, np.sort(rng.choice(z100, 50)))]
    for z, ts in cases:
        seg = torch.full((len(z) + 6,), -7, dtype=torch.int32, device="cuda")
        td = dev(ts) if len(ts) else None
        rc = lib.mfgm_sparse_batch_seg(len(z), dev(z).data_ptr(), len(ts), None if td is None else td.data_ptr(), seg.data_ptr(), None)
        assert rc == 0
        torch.cuda.synchronize()
        got = host(seg)
        want = MB.batch_seg(z, ts)
        assert np.array_equal(got[:len(z) + 2], want) and (got[len(z) + 2:] == -7).all()
        fin = ts[np.isfinite(ts)]
        assert np.array_equal(np.diff(want)[:-1], np.bincount(S.gaps(fin, z)[0], minlength=len(z) + 1)[:-1])      # the intervals of idx


# ---- 3 - 5. the model --------------------------------------------------------------------------------------------------------------------------
M_M = 12


def _lik(name):
    from vidp_amd.likelihoods import Bernoulli, Gaussian, Poisson
    return {"gaussian": Gaussian, "bernoulli": Bernoulli, "poisson": Poisson}[name](LIKS[name][1])


def _problem(rng, spec, N, lik):
    z, t, y = S.make_problem(rng, spec, M_M, N, "poisson" if lik == "poisson" else "gaussian")
    if lik == "bernoulli":
        y = (y > 0).astype(np.float64)
    return z, t, y


def _model(spec, jitter, z, lik, num_data=None, mean=None, lr=0.5):
    from vidp_amd.mean_function import LinearMeanFunction
    from vidp_amd.sparse_variational_cvi import SparseCVIGaussianProcess
    mf = None if mean is None else LinearMeanFunction(mean)
    return SparseCVIGaussianProcess(H.build_vidp(spec, jitter), dev(z), _lik(lik), mean_function=mf, learning_rate=lr, num_data=num_data)


def _batch(t, y, sel):
    return dev(t[sel]), dev(y[sel][:, None])


@pytest.mark.parametrize("mean", [None, 0.15], ids=["zero_mean", "linear_mean"])
@pytest.mark.parametrize("tree", ["matern52", "sum_m52_m32", "prod_m32_h"])
def test_one_epoch_is_the_full_batch(amd, rng, tree, mean):
    """Gaussian likelihood (its site gradients do not depend on q): M = 12, N = 60, four disjoint shuffled batches of 15, num_data = 60,
    rho_k = 1 / k.  After the four updates nat1 and nat2 are those of ONE full-batch update at learning rate 1 of a model without
    num_data, within 1e-12 of the largest site entry (the two differ in the order of sums over at most 60 terms)."""
    spec, jitter = TREES[tree]
    z, t, y = _problem(rng, spec, 60, "gaussian")
    full = _model(spec, jitter, z, "gaussian", mean=mean, lr=1.0)
    full.update_sites((dev(t), dev(y[:, None])))
    m = _model(spec, jitter, z, "gaussian", num_data=60, mean=mean)
    assert m._batch_native(dev(t))
    perm = rng.permutation(60)
    for k in range(4):
        m.learning_rate = 1.0 / (k + 1)
        m.update_sites(_batch(t, y, perm[15 * k:15 * (k + 1)]))
    m.dist_p.plan.check_info()
    e1, e2 = of_largest(host(m.nat1), host(full.nat1)), of_largest(host(m.nat2), host(full.nat2))
    print(f"{tree} mean {mean}: one epoch against the full batch nat1 {e1:.2e}, nat2 {e2:.2e} (bound {FULL_TOL:.0e})")
    assert e1 <= FULL_TOL and e2 <= FULL_TOL
    assert getattr(m, "_data_cache", None) is None          # no batch was kept as a data set


def _start_sites(spec, jitter, z, t, y, lik):
    """Non-trivial sites: one damped full-data step of the restatement from zero."""
    c = MB.BatchChain(spec, jitter, z, t, y, LIKS[lik], len(t))
    return c.update_sites(*c.zero_sites(), 0.5)


@pytest.mark.parametrize("lik", ["poisson", "bernoulli"])
@pytest.mark.parametrize("tree", ["matern52", "sum_m52_m32"])
def test_minibatch_steps_against_restatement(amd, rng, tree, lik):
    """Two mini-batch steps (n = 20 of N = 40, lr = 0.5) from non-trivial sites: the sites within 1e-10 of the largest entry and
    classic_elbo(batch) within 1e-9 of the restatement run on the same batches.  Then the whole data set as ONE shuffled batch with
    num_data = N against the sorted full-batch route of the same class: sites and bound within 1e-12.  And the Stamp rules: the data
    pass of classic_elbo serves an update_sites on the same batch object; after it the sites have moved and it is made again."""
    spec, jitter = TREES[tree]
    N = 40
    z, t, y = _problem(rng, spec, N, lik)
    n1, n2 = _start_sites(spec, jitter, z, t, y, lik)
    m = _model(spec, jitter, z, lik, num_data=N)
    m.nat1, m.nat2 = dev(n1), dev(n2)
    perm = rng.permutation(N)
    for k in range(2):
        sel = perm[20 * k:20 * (k + 1)]
        batch = _batch(t, y, sel)
        c = MB.BatchChain(spec, jitter, z, t[sel], y[sel], LIKS[lik], N)
        got, want = float(m.classic_elbo(batch)), c.elbo(n1, n2)
        kept = m._batch_cache
        m.update_sites(batch)
        assert m._batch_cache is kept                       # the ELBO's data pass served the update
        n1, n2 = c.update_sites(n1, n2, 0.5)
        e0, e1, e2 = abs(got - want) / abs(want), of_largest(host(m.nat1), n1), of_largest(host(m.nat2), n2)
        print(f"{tree}-{lik} step {k}: elbo {e0:.2e} (bound {ELBO_TOL:.0e}), nat1 {e1:.2e}, nat2 {e2:.2e} (bound {SITE_TOL:.0e})")
        assert e0 <= ELBO_TOL and e1 <= SITE_TOL and e2 <= SITE_TOL
        after = float(m.classic_elbo(batch))
        assert m._batch_cache is not kept and abs(after - c.elbo(n1, n2)) <= ELBO_TOL * abs(after)
    m.dist_p.plan.check_info()
    # one whole shuffled batch against the sorted full-batch route
    full = _model(spec, jitter, z, lik)
    full.nat1, full.nat2 = m.nat1.clone(), m.nat2.clone()
    whole, data = _batch(t, y, rng.permutation(N)), (dev(t), dev(y[:, None]))
    ea = abs(float(m.classic_elbo(whole)) - float(full.classic_elbo(data))) / abs(float(full.classic_elbo(data)))
    m.update_sites(whole)
    full.update_sites(data)
    e1, e2 = of_largest(host(m.nat1), host(full.nat1)), of_largest(host(m.nat2), host(full.nat2))
    print(f"{tree}-{lik}: whole batch against the full-batch route elbo {ea:.2e}, nat1 {e1:.2e}, nat2 {e2:.2e} (bound {FULL_TOL:.0e})")
    assert ea <= FULL_TOL and e1 <= FULL_TOL and e2 <= FULL_TOL


@pytest.mark.parametrize("lik", ["gaussian", "poisson", "bernoulli"])
@pytest.mark.parametrize("tree", ["matern32", "prod_m32_h"])
def test_torch_route_equals_native(amd, rng, monkeypatch, tree, lik):
    """VIDP_NATIVE_MINIBATCH=0 against the native route on the same two batches (one of them with a linear mean function in play):
    sites and bound within 5e-12 relative to max(1, |x|)."""
    spec, jitter = TREES[tree]
    N = 40
    z, t, y = _problem(rng, spec, N, lik)
    perm = rng.permutation(N)
    batches = [_batch(t, y, perm[:24]), _batch(t, y, perm[24:])]        # (the second, smaller batch carries its own scale)
    res = []
    for native in (True, False):
        if not native:
            monkeypatch.setenv("VIDP_NATIVE_MINIBATCH", "0")
        m = _model(spec, jitter, z, lik, num_data=N, mean=0.1)
        assert m._batch_native(batches[0][0]) == native
        e = []
        for b in batches:
            m.update_sites(b)
            e.append(float(m.classic_elbo(b)))
        res.append((host(m.nat1), host(m.nat2), np.array(e)))
    errs = [rel(a, b) for a, b in zip(res[1], res[0])]
    print(f"{tree}-{lik}: torch route against native nat1 {errs[0]:.2e}, nat2 {errs[1]:.2e}, elbo {errs[2]:.2e} (bound {ROUTE_TOL:.0e})")
    assert max(errs) <= ROUTE_TOL


def test_wide_tree_takes_the_torch_route(amd, rng):
    """The d = 9 Sum of three Matern-5/2 (wide plan, packed sites) is outside the native rows: two Poisson mini-batch steps on the torch
    route against the restatement, the bounds of test 4."""
    N, lik = 40, "poisson"
    z, t, y = _problem(rng, SUM9, N, lik)
    m = _model(SUM9, 0.0, z, lik, num_data=N)
    assert not m._batch_native(dev(t))
    n1, n2 = MB.BatchChain(SUM9, 0.0, z, t, y, LIKS[lik], N).zero_sites()
    perm = rng.permutation(N)
    for k in range(2):
        sel = perm[20 * k:20 * (k + 1)]
        batch = _batch(t, y, sel)
        c = MB.BatchChain(SUM9, 0.0, z, t[sel], y[sel], LIKS[lik], N)
        m.update_sites(batch)
        n1, n2 = c.update_sites(n1, n2, 0.5)
        got, want = float(m.classic_elbo(batch)), c.elbo(n1, n2)
        e0, e1, e2 = abs(got - want) / abs(want), of_largest(host(m.nat1), n1), of_largest(host(m.nat2), n2)
        print(f"sum9 step {k}: elbo {e0:.2e} (bound {ELBO_TOL:.0e}), nat1 {e1:.2e}, nat2 {e2:.2e} (bound {SITE_TOL:.0e})")
        assert e0 <= ELBO_TOL and e1 <= SITE_TOL and e2 <= SITE_TOL


def test_update_sites_makes_no_host_synchronisation(amd, rng):
    """After a first step (which builds the prior and the plan), update_sites on a new unsorted batch runs with torch's
    synchronisation check set to raise: the native route never looks at the data on the host."""
    import torch
    spec, jitter = TREES["sum_m52_m32"]
    z, t, y = _problem(rng, spec, 40, "poisson")
    m = _model(spec, jitter, z, "poisson", num_data=400, mean=0.1)
    perm = rng.permutation(40)
    m.update_sites(_batch(t, y, perm[:20]))
    batch = _batch(t, y, perm[20:])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m.update_sites(batch)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.isfinite(host(m.nat1)).all()


# ---- 6. out of scope -----------------------------------------------------------------------------------------------------------------------------
def test_out_of_scope_raises(amd, rng):
    """num_data with shard=, and elbo_and_grad in mini-batch mode, raise NotImplementedError; the models built on the class do not
    take the keyword."""
    from vidp_amd import kernels as K
    from vidp_amd.likelihoods import Gaussian
    from vidp_amd.panel_variational_cvi import PanelSparseCVI
    from vidp_amd.sparse_variational_cvi import SparseCVIGaussianProcess
    with pytest.raises(NotImplementedError):
        SparseCVIGaussianProcess(H.build_vidp(SUM9), dev(np.linspace(0.0, 100.0, 200)), Gaussian(1.0), num_data=1000,
                                 shard=dict(rank=0, world=2, allreduce=lambda x: x, allgather=lambda x: x[None]))
    m = SparseCVIGaussianProcess(K.Matern32(1.0, 1.0), dev(np.linspace(0.0, 5.0, 8)), Gaussian(1.0), num_data=100)
    data = (dev(np.linspace(0.1, 4.9, 10)), dev(rng.normal(size=(10, 1))))
    with pytest.raises(NotImplementedError):
        m.elbo_and_grad(data)
    with pytest.raises(ValueError):
        SparseCVIGaussianProcess(K.Matern32(1.0, 1.0), dev(np.linspace(0.0, 5.0, 8)), Gaussian(1.0), num_data=0)
    with pytest.raises(TypeError):
        PanelSparseCVI(K.Matern32(1.0, 1.0), dev(np.linspace(0.0, 5.0, 8)), Gaussian(1.0), num_data=100)


# ---- 7. the trainer -------------------------------------------------------------------------------------------------------------------------------
def test_trainer_is_reproducible_and_raises_the_elbo(amd, rng):
    """Poisson, M = 12, N = 240, batches of 40, three epochs (18 steps) at rho_k = 1 / k: the same seed gives the same batches and
    bit-identical sites on two runs, another seed other batches; the full-data classic_elbo of a num_data=None twin that carries the
    trained sites is higher than at the zero sites.  N = 250 with batches of 40: the last batch of an epoch has 10 points."""
    import torch
    import vidp_amd
    spec, jitter = TREES["matern52"]
    N = 240
    z, t, y = _problem(rng, spec, N, "poisson")
    data = (dev(t), dev(y[:, None]))

    def run(seed):
        m = _model(spec, jitter, z, "poisson", num_data=N)
        tr = vidp_amd.MiniBatchSitesTrainer(m, data, batch_size=40, seed=seed)
        first = tr.next_batch()[0].clone()
        tr = vidp_amd.MiniBatchSitesTrainer(m, data, batch_size=40, seed=seed)
        tr.fit(18)
        assert tr.k == 18 and m.learning_rate == 1.0 / 18
        return m, first, float(tr.elbo_estimate())

    m1, b1, e1 = run(5)
    m2, b2, e2 = run(5)
    _, b3, _ = run(6)
    assert torch.equal(b1, b2) and not torch.equal(b1, b3)
    assert torch.equal(m1.nat1, m2.nat1) and torch.equal(m1.nat2, m2.nat2) and e1 == e2
    twin = _model(spec, jitter, z, "poisson")
    before = float(twin.classic_elbo(data))
    twin.nat1, twin.nat2 = m1.nat1.clone(), m1.nat2.clone()
    after = float(twin.classic_elbo(data))
    print(f"trainer: full-data elbo {before:.3f} at the zero sites -> {after:.3f} after three epochs; last batch estimate {e1:.3f}")
    assert after > before
    # the smaller last batch of an epoch
    z, t, y = _problem(rng, spec, 250, "poisson")
    tr = vidp_amd.MiniBatchSitesTrainer(_model(spec, jitter, z, "poisson", num_data=250), (dev(t), dev(y[:, None])), batch_size=40, seed=1)
    sizes, seen = [], []
    for _ in range(8):
        tr.step()
        sizes.append(int(tr.last_batch[0].shape[0]))
        seen.append(host(tr.last_batch[0]))
    assert sizes == [40] * 6 + [10, 40]
    assert np.array_equal(np.sort(np.concatenate(seen[:7])), np.sort(t))          # an epoch is every point once
