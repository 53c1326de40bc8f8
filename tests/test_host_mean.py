"""
Host tests (no GPU) of the mean functions (vidp_amd.mean_function): the reference's known answers (tests/unit/test_mean_function.py)
on the torch route and on the long-double restatement tests/np_mean.py; expm(G dt) against the closed-form transitions of every kernel
tree the GPU test uses (the precondition of a_k = -G^-1 u_k); constructor errors; ties and K = 1; the torch route against the
restatement; the argument checks of the two native entry points, which return before any HIP call.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import np_kernels
from tests import np_kernels_ext as E
from tests import np_mean as NM

EXPECTED_RANGE = 12.0
K_ACTIONS = 5


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))


@pytest.fixture(scope="module")
def mf():
    import vidp_amd.mean_function as mf
    return mf


@pytest.fixture(scope="module")
def K():
    from vidp_amd import kernels
    return kernels


def _setup(rng, batch_shape, K, num=K_ACTIONS, lengthscale=1.0):
    gk, ok = K.Matern32(lengthscale, 1.0), np_kernels.Matern32(lengthscale, 1.0)
    u = rng.normal(size=batch_shape + (num, 2))
    t = np.sort(rng.uniform(0.0, EXPECTED_RANGE, size=batch_shape + (num,)), axis=-1)
    return gk, ok, t, u


class Restated:
    """The restatement behind the mean functions' call signature: [..., N] -> [..., N, 1], chain by chain."""

    def __init__(self, kind, ok, t, u):
        self.kind, self.ok, self.t, self.u = kind, ok, t, u

    def __call__(self, tq):
        tq = np.broadcast_to(tq, self.t.shape[:-1] + tq.shape[-1:])
        out = np.zeros(tq.shape + (1,))
        for ix in np.ndindex(*self.t.shape[:-1]):
            out[ix][:, 0] = NM.mean(self.ok, self.kind, self.t[ix], self.u[ix], tq[ix])["f"].astype(np.float64)
        return out


def both(kind, mf, gk, ok, t, u):
    cls = mf.ImpulseMeanFunction if kind == "impulse" else mf.StepMeanFunction
    m = cls(T(t), T(u), gk)
    return [lambda tq: m(T(tq)).numpy(), Restated(kind, ok, t, u)]


def test_impulse_known_answers(rng, batch_shape, mf, K):
    gk, ok, t, u = _setup(rng, batch_shape, K)
    fu = u[..., :1]                                                     # H u with H = [1, 0]
    for f in both("impulse", mf, gk, ok, t, u):
        np.testing.assert_allclose(f(t - 1e-15) + fu, f(t + 1e-15), rtol=0, atol=1e-10)       # the jump is H u_k
        np.testing.assert_allclose(f(t - 1e-15), f(t), rtol=0, atol=1e-10)                     # not yet seen on t_k
        np.testing.assert_allclose(f(t + 10 * EXPECTED_RANGE), 0.0, rtol=0, atol=1e-10)        # decayed 120 later
        np.testing.assert_array_equal(f(t[..., :1] - 1e-6), 0.0)                               # zero before the first


def test_step_known_answers(rng, batch_shape, mf, K):
    gk, ok, t, u = _setup(rng, batch_shape, K)
    for f in both("step", mf, gk, ok, t, u):
        np.testing.assert_allclose(f(t - 1e-15), f(t + 1e-15), rtol=0, atol=1e-10)             # continuous across a step
        np.testing.assert_allclose(f(t - 1e-15), f(t), rtol=0, atol=1e-10)
        np.testing.assert_array_equal(f(t[..., :1] - 1e-6), 0.0)


def test_far_from_step(rng, batch_shape, mf, K):
    """A long way after each step the state has settled on -F^-1 u_k."""
    gk, ok = K.Matern32(3.0, 1.0), np_kernels.Matern32(3.0, 1.0)
    t = np.broadcast_to(np.arange(3) * 100.0 - 10.0, batch_shape + (3,)).copy()
    u = rng.normal(size=batch_shape + (3, 2))
    far = np.einsum("ij,...j->...i", -np.linalg.inv(ok.feedback_matrix()), u)[..., :1]
    for f in both("step", mf, gk, ok, t, u):
        np.testing.assert_allclose(f(t + 99.0), far, rtol=0, atol=1e-10)


def _expm(F, ts):
    return torch.linalg.matrix_exp(T(F)[None] * T(ts)[:, None, None]).numpy()


def test_single_impulse_and_step_closed_forms(mf, K):
    gk, ok = K.Matern32(3.0, 1.0), np_kernels.Matern32(3.0, 1.0)
    u = np.array([[2.3, 1.2]])
    tq = np.linspace(0.01, 12.0, 100)
    F = ok.feedback_matrix()
    eF = _expm(F, tq)
    expected = (eF @ u[0])[:, :1]                                        # mu(t) = expm(F t) u
    for f in both("impulse", mf, gk, ok, np.zeros(1), u):
        np.testing.assert_allclose(f(tq), expected, rtol=1e-7)
    Finv_u = np.linalg.solve(F, u[0])
    expected = (-Finv_u + eF @ Finv_u)[:, :1]                            # mu(t) = -F^-1 u + expm(F t) F^-1 u
    for f in both("step", mf, gk, ok, np.zeros(1), u):
        np.testing.assert_allclose(f(tq), expected, rtol=1e-7)


def test_zero_and_linear_are_exact(batch_shape, rng, mf):
    t = T(rng.uniform(0.0, 10.0, size=batch_shape + (7,)))
    z = mf.ZeroMeanFunction(obs_dim=2)(t)
    assert tuple(z.shape) == batch_shape + (7, 2) and bool((z == 0).all()) and z.dtype == t.dtype
    lin = mf.LinearMeanFunction(1.7, obs_dim=3)(t)
    assert tuple(lin.shape) == batch_shape + (7, 3)
    assert torch.equal(lin, (1.7 * t)[..., None].expand(batch_shape + (7, 3)))
    assert torch.equal(mf.LinearMeanFunction(-0.5)(t), -0.5 * t[..., None])
    assert not mf.ZeroMeanFunction(1).depends_on_kernel and not mf.LinearMeanFunction(1.0).depends_on_kernel
    assert mf.ImpulseMeanFunction.depends_on_kernel and mf.StepMeanFunction.depends_on_kernel


@pytest.mark.parametrize("d", range(1, 9))
def test_generator_reproduces_the_closed_form_transitions(d, K):
    """expm(G dt) = transition_statistics_local(dt)[0] with G = kernel.generator_matrix: what a_k = -G^-1 u_k rests on.  G is the
    feedback matrix for every tree without a Product; a Product's feedback_matrix is the reference's Kronecker product and does NOT
    generate its transitions (the Kronecker sum does), so the step mean solves against generator_matrix."""
    gk, ok = NM.tree(d, K, K), NM.tree(d, np_kernels, E)
    dt = T(np.array([0.0, 1e-3, 0.37, 2.9]))
    A = gk.transition_statistics_local(dt)[0]
    G = gk.generator_matrix
    np.testing.assert_allclose(torch.linalg.matrix_exp(G[None] * dt[:, None, None]).numpy(), A.numpy(), rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(G.numpy(), NM.generator(ok).astype(np.float64), rtol=1e-15, atol=0)
    if d in (1, 2, 3, 4, 7):
        assert torch.equal(G, gk.feedback_matrix)
    else:
        assert not torch.allclose(torch.linalg.matrix_exp(gk.feedback_matrix * 0.37), A[2], rtol=1e-3, atol=1e-3)


def test_constructor_errors(mf, K):
    k = K.Matern32(1.0, 1.0)
    t, u = torch.tensor([0.0, 1.0, 2.0], dtype=torch.float64), torch.zeros((3, 2), dtype=torch.float64)
    for cls in (mf.ImpulseMeanFunction, mf.StepMeanFunction):
        with pytest.raises(ValueError, match="non-decreasing"):
            cls(torch.tensor([0.0, 2.0, 1.0], dtype=torch.float64), u, k)
        with pytest.raises(ValueError, match="state_perturbations"):
            cls(t, torch.zeros((4, 2), dtype=torch.float64), k)
        with pytest.raises(ValueError, match="state_dim"):
            cls(t, torch.zeros((3, 3), dtype=torch.float64), k)
        with pytest.raises(ValueError, match="at least one action"):
            cls(t[:0], u[:0], k)
        pw = K.PiecewiseKernel([K.Matern32(1.0, 1.0), K.Matern32(2.0, 1.0)], torch.tensor([0.5], dtype=torch.float64))
        with pytest.raises(NotImplementedError, match="PiecewiseKernel"):
            cls(t, u, pw)
    const = K.Product([K.Constant(2.0)])
    with pytest.raises(ValueError, match="Product"):
        mf.StepMeanFunction(t, torch.zeros((3, 1), dtype=torch.float64), const)
    with pytest.raises(ValueError, match="Sum"):
        mf.StepMeanFunction(t, torch.zeros((3, 3), dtype=torch.float64), K.Sum([K.Matern32(1.0, 1.0), K.Constant(1.0)], jitter=1e-6))
    mf.ImpulseMeanFunction(t, torch.zeros((3, 1), dtype=torch.float64), const)          # impulses need no inverse
    mf.StepMeanFunction(torch.tensor([0.0, 0.0, 2.0], dtype=torch.float64), u, k)       # ties are allowed


def _relative_to_scale(got, ref, scale):
    """max |got - ref| / scale over the entries with a positive scale; entries whose scale is zero must be exactly zero."""
    got, ref, scale = np.asarray(got, dtype=NM.LD), np.asarray(ref), np.asarray(scale)
    assert np.all(got[scale == 0] == 0)
    pos = scale > 0
    return float(np.max(np.abs(got - ref)[pos] / scale[pos])) if pos.any() else 0.0


# The torch route rounds each transition entry (a few ulp), each of the d fma of a mat-vec row and, for the steps, the fp64 solve
# against G (cond(G) < 1e3 on these trees, against the long-double solve of the restatement): 1e-12 of the absolute-value recurrence,
# the bound of the device kernels, leaves two orders of magnitude.
TORCH_ROUTE_BOUND = 1e-12


@pytest.mark.parametrize("kind", ["impulse", "step"])
@pytest.mark.parametrize("d", range(1, 9))
def test_torch_route_against_the_restatement(d, kind, rng, mf, K):
    gk, ok = NM.tree(d, K, K), NM.tree(d, np_kernels, E)
    cls = mf.ImpulseMeanFunction if kind == "impulse" else mf.StepMeanFunction
    for Kn in (1, 9):
        t = np.cumsum(rng.uniform(0.0, 0.6, size=(2, Kn)), axis=-1)
        if Kn > 3:
            t[:, 3] = t[:, 2]                                             # a tie
        u = rng.normal(size=(2, Kn, d))
        tq = np.concatenate([t, np.nextafter(t, np.inf), t[:, :1] - 1.0, t[:, -1:] + 30.0, rng.uniform(t.min(), t.max(), size=(2, 20))],
                            axis=-1)
        m = cls(T(t), T(u), gk)
        state, f = m.state_mean(T(tq)).numpy(), m(T(tq)).numpy()
        assert state.shape == (2, tq.shape[-1], d) and f.shape == (2, tq.shape[-1], 1)
        for b in range(2):
            ref = NM.mean(ok, kind, t[b], u[b], tq[b])
            assert _relative_to_scale(state[b], ref["mu"], ref["mu_scale"]) < TORCH_ROUTE_BOUND
            assert _relative_to_scale(f[b, :, 0], ref["f"], ref["f_scale"]) < TORCH_ROUTE_BOUND
            # on an action time the action is not yet seen: the value of the actions strictly before it alone (exactly zero when
            # there is none: the scale is zero there)
            for k in range(Kn):
                j = int(np.searchsorted(t[b], t[b, k], side="left"))
                if j > 0:
                    rj = NM.mean(ok, kind, t[b, :j], u[b, :j], t[b, k:k + 1])
                    assert _relative_to_scale(state[b, k], rj["mu"][0], rj["mu_scale"][0]) < TORCH_ROUTE_BOUND


def test_cache_follows_the_kernel_and_the_actions(mf, K):
    k = K.Matern32(1.0, 1.0)
    t, u = torch.tensor([0.0, 1.0], dtype=torch.float64), torch.tensor([[1.0, 0.0], [0.5, -1.0]], dtype=torch.float64)
    m = mf.StepMeanFunction(t, u, k)
    tq = torch.tensor([0.5, 1.5, 4.0], dtype=torch.float64)
    a = m(tq)
    assert m._coefficients(tq.device) is m._coefficients(tq.device)
    k.assign_hyperparameters({"lengthscale": 2.0, "variance": 1.0})
    b = m(tq)                                                             # the key holds the kernel's values: no stale coefficients
    assert not torch.equal(a, b)
    assert torch.equal(b, mf.StepMeanFunction(t, u, K.Matern32(2.0, 1.0))(tq))
    u.mul_(2.0)                                                           # an in-place edit of the perturbations moves the stamp
    assert torch.allclose(m(tq), 2.0 * b, rtol=1e-14, atol=0)
    m.kernel_changed()
    assert m._cache == {}


def test_leg_kernel_takes_the_torch_route(mf, K, rng):
    N, R = T(rng.normal(size=(3, 3))), T(rng.normal(size=(3, 3)))
    k = K.LatentExponentiallyGenerated(N, R)
    t, u = T(np.array([0.0, 0.4, 1.1])), T(rng.normal(size=(3, 3)))
    m = mf.StepMeanFunction(t, u, k)
    tq = T(np.array([0.2, 0.4, 0.9, 3.0]))
    F = k.feedback_matrix
    a = -torch.linalg.solve(F, u.T).T
    # piecewise closed form: mu' = F mu + u_k  =>  mu(t) = a_k + expm(F (t - t_k)) (mu(t_k) - a_k)
    out = []
    for q in tq.tolist():
        mu_q, last = torch.zeros(3, dtype=torch.float64), None
        for i in range(3):
            if float(t[i]) < q:
                if last is not None:
                    mu_q = a[last] + torch.linalg.matrix_exp(F * (float(t[i]) - float(t[last]))) @ (mu_q - a[last])
                last = i
        if last is not None:
            mu_q = a[last] + torch.linalg.matrix_exp(F * (q - float(t[last]))) @ (mu_q - a[last])
        out.append(mu_q)
    np.testing.assert_allclose(m.state_mean(tq).numpy(), torch.stack(out).numpy(), rtol=1e-10, atol=1e-12)


def test_entry_points_refuse_bad_arguments_without_a_device(K):
    import vidp_amd
    lib = vidp_amd._lib.load()
    kt = NM.tree(3, K, K)._terms_struct()
    p = ctypes.c_void_p(8)          # never dereferenced: every call below returns before any HIP call
    coefficients = lambda terms, B, Kn, seg, *ptrs: lib.mfgm_action_coefficients(terms, B, Kn, seg, *ptrs, None)
    assert coefficients(None, 1, 4, 0, p, p, p, p) == 1
    for missing in range(4):
        ptrs = [p] * 4
        ptrs[missing] = None
        assert coefficients(ctypes.byref(kt), 1, 4, 0, *ptrs) == 1
    assert coefficients(ctypes.byref(kt), 1, 0, 0, p, p, p, p) == 1            # K = 0
    assert coefficients(ctypes.byref(kt), 0, 4, 0, p, p, p, p) == 1            # B = 0
    assert coefficients(ctypes.byref(kt), 1, 4, -1, p, p, p, p) == 1
    mean = lambda terms, B, Kn, N, *ptrs: lib.mfgm_action_mean(terms, B, Kn, N, *ptrs, None)
    assert mean(None, 1, 4, 3, p, p, None, p, p, p, p) == 1
    assert mean(ctypes.byref(kt), 1, 4, 3, None, p, None, p, p, p, p) == 1
    assert mean(ctypes.byref(kt), 1, 4, 3, p, None, None, p, p, p, p) == 1
    assert mean(ctypes.byref(kt), 1, 4, 3, p, p, None, None, p, p, p) == 1     # no query points
    assert mean(ctypes.byref(kt), 1, 4, 3, p, p, None, p, None, p, p) == 1     # f_mean without an emission row
    assert mean(ctypes.byref(kt), 1, 0, 3, p, p, None, p, p, p, p) == 1        # K = 0
    assert mean(ctypes.byref(kt), 0, 4, 3, p, p, None, p, p, p, p) == 1
    assert mean(ctypes.byref(kt), 1, 4, 0, p, p, None, None, None, None, None) == 0      # N = 0: nothing to do
    # d = 9: three Matern-5/2 blocks
    k9 = K.Sum([K.Matern52(1.0, 1.0), K.Matern52(2.0, 1.0), K.Matern52(3.0, 1.0)])
    kt9 = vidp_amd._lib.KernelTerms()
    kt9.nterm = 3
    for c in range(3):
        kt9.nfactor[c], kt9.offset[c] = 1, 3 * c
        kt9.kind[c][0], kt9.rate[c][0], kt9.var[c][0] = vidp_amd._lib.FACTOR_MATERN52, 1.0 + c, 1.0
    assert k9.state_dim == 9
    assert coefficients(ctypes.byref(kt9), 1, 4, 0, p, p, p, p) == 1
    assert mean(ctypes.byref(kt9), 1, 4, 3, p, p, None, p, p, p, p) == 1
    # the workspace: B S d with S = ceil(K / seg_len), seg_len = 0 -> the smallest s with s s >= K
    ws = lib.mfgm_action_workspace_doubles
    assert ws(2, 70, 3, 0) == 2 * math.ceil(70 / 9) * 3 and ws(2, 70, 3, 4) == 2 * 18 * 3 and ws(1, 5, 8, 64) == 8
    assert ws(1, 100000, 3, 0) == math.ceil(100000 / 317) * 3
    assert ws(1, 0, 3, 0) == 0 and ws(1, 4, 9, 0) == 0 and ws(0, 4, 3, 0) == 0
