"""
Host tests (no GPU) of tests/np_vdp.py, the 80-bit reference and input generator of tests/test_gpu_vdp.py: the fp64 twins reproduce
oracle/np_models.VariationalMarkovGP to rounding in the settings the oracle can express, the per-dimension gradients of the energy
agree with central differences of the energy, every generator condition holds for every d = 1 ... 8, shape and variant, and the
yardsticks (fp64 twin against the 80-bit reference) of every output are printed: the table tests/test_gpu_vdp.py cites.
"""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import np_vdp
from tests.np_vdp import LD

DIMS = list(range(1, 9))
VARIANTS = ["full", "noobs", "clip", "stab"]
# two fp64 evaluations of the same recurrences in another order of operations (the oracle's einsum / matmul forms against the twin's):
# a few eps per node over the 32 transitions of the shape used, entries of order one
ROUNDING = 1e-13


def close(name, got, want):
    err = np_vdp.rel_err(got, want)
    print(f"  {name}: twin against the oracle {err:.3e}")
    assert err <= ROUNDING, (name, err)


@pytest.mark.parametrize("stab", [False, True], ids=["plain", "stabilised"])
@pytest.mark.parametrize("d", [1, 2, 3, 6, 8])
def test_twins_reproduce_the_oracle(d, stab):
    """forward_pass, _grad_E_sde, update_lagrange, update_param of np_models.VariationalMarkovGP(closed_form=True) against the fp64 twins:
    scalar af, bf, a diagonal q with distinct entries, one observation per node at nodes the loop reads (1, 2, 8, T-2), a dense R.
    Stabilised: the forward pass on the "stab" inputs (NaN entries, transitions and offsets beyond [-1, 1]), the Lagrange sweep and the
    parameter update on the ordinary inputs with the oracle's CLIP_MIN / CLIP_MAX set to -+0.3."""
    from oracle import np_models, np_sde
    f64 = np.float64
    shape = np_vdp.SHAPES[1]
    case = np_vdp.make_case(d, shape, "full")
    T, dt = case.T, case.prm.dt
    scale, c = 0.7, 1.3
    sde = np_sde.DoubleWellSDE(q=np.diag(case.prm.q), scale=scale, c=c)
    prm = SimpleNamespace(**vars(case.prm))
    prm.af, prm.bf = np.full(d, scale * c), np.full(d, scale)
    prm.clip = 0.3 if stab else 0.0          # below every entry of -1/2 R^-1's diagonal (R^-1 >= 1 there) and part of everything else
    rng = np.random.default_rng(d)
    cholR = np.tril(0.3 * rng.normal(size=(d, d)), -1) + np.diag(0.6 + 0.4 * rng.random(d))
    lik = np_models.MultivariateGaussianLik(cholR)
    idx = np.array([1, 2, 8, T - 2])
    y = rng.normal(size=(len(idx), d))
    yR, dobsS = np.zeros((1, T, d)), np.zeros((1, T, d, d))
    yR[0, idx], dobsS[0, idx] = y @ lik.inv_cov, -0.5 * lik.inv_cov
    grid = np.arange(T) * dt

    def oracle(A, b):
        o = np_models.VariationalMarkovGP(idx, y, sde, grid, lik, np.zeros(d), np.eye(d), stabilize_system=stab, closed_form=True)
        o.A, o.b = A[0].copy(), b[0].copy()
        o.q0_mu, o.q0_chol = case.q0_mu[0].copy(), np.linalg.cholesky(case.q0_cov[0])
        return o

    # forward pass
    fwd = np_vdp.make_case(d, shape, "stab") if stab else case
    o = oracle(fwd.A, fwd.b)
    m, S = o.forward_pass()
    pf = SimpleNamespace(**vars(prm))
    pf.clip = fwd.prm.clip
    tm, tS, _ = np_vdp.marginals(fwd.A, fwd.b, pf, case.q0_mu, o.q0_chol @ o.q0_chol.T, f64)
    close("m", tm[0], m)
    close("S", tS[0], S)
    # energy, its gradients, the Lagrange sweep and the parameter update on the ordinary inputs
    o = oracle(case.A, case.b)
    o.CLIP_MIN, o.CLIP_MAX = -prm.clip, prm.clip
    m, S = (x[0] for x in np_vdp.marginals(case.A, case.b, SimpleNamespace(**{**vars(prm), "clip": 0.0}), case.q0_mu, case.q0_cov, f64)[:2])
    e, gm, gS = np_vdp.esde(m[None], S[None], case.A, case.b, prm, f64)
    want_m, want_S = o._grad_E_sde(m, S)
    close("E_sde", e[0] * dt, o.E_sde(m[:-1], S[:-1]))
    close("dE/dm", gm[0], want_m)
    close("dE/dS", gS[0], want_S)
    lg = np_vdp.lagrange(m[None], S[None], case.A, case.b, prm, yR, dobsS, f64)
    o.update_lagrange(m, S)
    close("psi", lg.psi[0], o.psi)
    close("lam", lg.lam[0], o.lam)
    if stab:
        # the four quantities are clipped, each on its own
        for name, x in lg.pre.items():
            assert np.abs(x).max() > prm.clip, name
    for lr in np_vdp.LRS:
        o2 = oracle(case.A, case.b)
        o2.psi, o2.lam = o.psi.copy(), o.lam.copy()
        pm = prm
        o2.CLIP_MIN, o2.CLIP_MAX = -pm.clip, pm.clip
        o2.update_param(m, S, lr)
        A2, b2, pc, lc = np_vdp.update_param(m[None], S[None], o.psi[None], o.lam[None], case.A, case.b, pm, lr, f64)
        close(f"lr={lr} A", A2[0], o2.A)
        close(f"lr={lr} b", b2[0], o2.b)
        np.testing.assert_array_equal(pc[0], o2.psi)
        np.testing.assert_array_equal(lc[0], o2.lam)
        if stab:
            assert np.abs(o.psi).max() > pm.clip and np.abs(o.lam).max() > pm.clip


@pytest.mark.parametrize("kind", ["dw", "ou"])
def test_energy_gradients_agree_with_central_differences(kind):
    """The 80-bit dE/dm, dE/dS (symmetric convention) against central differences of the 80-bit energy with h = 1e-5, to 1e-9 relative,
    at d = 3 with distinct af, bf, q: the one independent check of the per-dimension formulas (the oracle only sees scalar af, bf)."""
    d = 3
    case = np_vdp.make_case(d, np_vdp.SHAPES[1], "full", kind=kind)
    p, r = case.prm, case.ref
    assert len(set(p.af)) == len(set(p.q)) == d and (kind == "ou" or len(set(p.bf)) == d)
    N = case.T - 1
    m, S = r.m[:, :N].astype(LD), r.S[:, :N].astype(LD)
    energy = lambda mm, SS: np_vdp.energy_terms(mm, SS, case.A, case.b, p, LD, grads=False)[0]
    _, gm, gS = np_vdp.energy_terms(m, S, case.A, case.b, p, LD)
    h = LD(1e-5)
    fm, fS = np.zeros_like(gm), np.zeros_like(gS)
    for i in range(d):
        dm = np.zeros(d, dtype=LD)
        dm[i] = h
        fm[..., i] = (energy(m + dm, S) - energy(m - dm, S)) / (2 * h)
        for j in range(i + 1):
            dS = np.zeros((d, d), dtype=LD)
            dS[i, j] += h / 2
            dS[j, i] += h / 2
            fS[..., i, j] = fS[..., j, i] = (energy(m, S + dS) - energy(m, S - dS)) / (2 * h)
    for name, fd, g in (("dE/dm", fm, gm), ("dE/dS", fS, gS)):
        err = np_vdp.rel_err(fd, g)
        print(f"  {kind} {name}: central differences against the closed form {err:.3e}")
        assert err <= 1e-9, (name, err)


@pytest.mark.parametrize("shape", np_vdp.SHAPES, ids=np_vdp.SHAPE_IDS)
@pytest.mark.parametrize("d", DIMS)
def test_generator_conditions_and_yardsticks(d, shape):
    """make_case asserts every generator condition (np_vdp.check_case, np_vdp.clip_conditions); the yardstick of every output -- the
    fp64 twin against the 80-bit reference, as rel_err -- is printed, finite and below 1e-12."""
    for variant in VARIANTS:
        case = np_vdp.make_case(d, shape, variant)
        assert np_vdp.check_case(case, case.ref)
        if variant == "clip":
            print(f"  d={d} {shape} clip: prm.clip = {case.prm.clip}, update_param clip = {case.prm_m.clip}, seed {getattr(case, 'seed', 0)}")
        for name, y in np_vdp.yardsticks(case).items():
            print(f"  d={d} {shape} {variant} {name}: yardstick {y:.3e} ({y / np_vdp.EPS:.1f} eps)")
            assert np.isfinite(y) and y < 1e-12, (name, y)
    # per-dimension parameters are distinct, A is not symmetric, every off-diagonal entry of dobs_const is non-zero
    case = np_vdp.make_case(d, shape, "full")
    p = case.prm
    assert len(set(p.af)) == len(set(p.bf)) == len(set(p.q)) == d
    if d > 1:
        assert np.abs(case.A - np.swapaxes(case.A, -1, -2)).max() > 0.1 and np.abs(case.dobs_const[~np.eye(d, dtype=bool)]).min() > 0


def test_observation_edges_and_layout():
    """Observations sit at nodes 0, 1, 2, T-2, T-1, at the ends of a segment, one forced node and one random node carry two; "noobs" has
    none; obs_count packs like any one-entry node array."""
    shape = np_vdp.SHAPES[0]
    case = np_vdp.make_case(3, shape, "full")
    T, (n, R, P, Lpad) = case.T, case.levels[0]
    assert case.obs_count.max() == 2 and np.all((case.obs_count == 2).sum(axis=1) == 2)
    assert np.all(case.obs_count[:, case.twice] == 2) and (case.twice + 1) % R == 0
    assert np.all(case.obs_count.sum(axis=1) == case.obs_t.shape[1]) and np.all(case.obs_count.sum(axis=1) < T)
    np.testing.assert_array_equal(case.dobsS, case.obs_count[..., None, None] * case.dobs_const)
    assert np_vdp.make_case(3, shape, "noobs").obs_count.max() == 0
    flat = np_vdp.pack_nodes(case.obs_count[..., None], case.levels[0], np.array([7], dtype=np.int32))
    assert flat.dtype == np.int32 and flat.size == Lpad * R
    back, mask = np_vdp.unpack_nodes(flat, case.B, T, 1, case.levels[0])
    np.testing.assert_array_equal(back[..., 0], case.obs_count)
    assert np.all(flat[~mask] == 7)
