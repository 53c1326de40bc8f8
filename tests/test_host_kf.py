"""
Host tests of tests/np_kf.py, the 80-bit reference of the fused Kalman filter with sites (no GPU): that it restates the right
operation (against oracle.np_kalman.KalmanFilterWithSites, the project's fp64 restatement of the reference filter, and against the
dense marginal likelihood and posterior of one tiny case built in 80-bit), and that its own code run in float64 holds every bound of
tests/test_gpu_kf.py on every case that file uses -- so the bounds are attainable by honest fp64 arithmetic and no input needs
excluding.  The largest err / bound per output is printed (pytest -s) and copied into the docstring of tests/test_gpu_kf.py.
"""
import functools

import numpy as np
import pytest

from oracle import np_kalman, np_ssm
from tests import np_kf
from tests.helpers import random_ssm_params

LD = np_kf.LD


class _OneNodePrior:
    """The prior of a chain of one node, which oracle.np_ssm.StateSpaceModel refuses to build: what _Base.log_likelihood reads."""

    def __init__(self, mu0, cholP0):
        self.mu0, self.cholP0, self.num_transitions = mu0, cholP0, 0

    def precision(self):
        return np.linalg.inv(self.cholP0 @ np.swapaxes(self.cholP0, -1, -2))[..., None, :, :], None

    @property
    def marginal_means(self):
        return self.mu0[..., None, :]

    def log_det_precision(self):
        return -np.sum(np.log(np.square(np.diagonal(self.cholP0, axis1=-2, axis2=-1))), axis=-1)


@pytest.mark.parametrize("zero_mean", [False, True])
@pytest.mark.parametrize("T", [1, 2, 9])
@pytest.mark.parametrize("o", [1, 2])
@pytest.mark.parametrize("d", [1, 3, 8])
def test_right_operation_against_the_oracle(d, o, T, zero_mean):
    """total and the f-marginals of np_kf against the oracle filter on the precision of a random state-space model, B = 2, per-chain
    sites: 1e-10 relative.  (T = 1: the oracle cannot build a posterior state-space model of one node, so the marginals are held to
    the dense inverse instead.)"""
    B = 2
    rng = np.random.default_rng([991, d, o, T, int(zero_mean)])
    mu0, cholP0, A, b, cholQ = random_ssm_params(rng, (B,), max(T, 2), d)
    if zero_mean:
        mu0, b = np.zeros_like(mu0), np.zeros_like(b)
    ssm = np_ssm.StateSpaceModel(mu0, cholP0, A, b, cholQ) if T > 1 else _OneNodePrior(mu0, cholP0)
    Pd, Ps = ssm.precision()
    mu_p = None if zero_mean else np.array(ssm.marginal_means)
    cs = np_kf.make_case(d, o, B, T, False, zero_mean, prior=(Pd, Ps, mu_p, -0.5 * ssm.log_det_precision()))
    ref = np_kf.reference(cs)
    okf = np_kalman.KalmanFilterWithSites(ssm, np.broadcast_to(cs.H, (B, T, o, d)), np_kalman.GaussianSitesNat(cs.nat1, cs.nat2))
    want = okf.log_likelihood()
    assert abs(float(ref.total) - want) <= 1e-10 * abs(want), (float(ref.total), want)
    if T > 1:
        mu, cov = okf.posterior_state_space_model().marginals
    else:
        D = np.asarray(ref.m0.D, dtype=np.float64)[:, 0]
        cov = np.linalg.inv(D)[:, None]
        mu = np.einsum("btij,btj->bti", cov, np.asarray(ref.m1.r, dtype=np.float64))
    Fmu, Fvar = np.einsum("ai,bti->bta", cs.H, mu), np.einsum("ai,aj,btij->bta", cs.H, cs.H, cov)
    for got, w in ((ref.Fmu, Fmu), (ref.Fvar, Fvar), (ref.x, mu), (ref.Sig, cov)):
        assert np.max(np.abs(np.asarray(got, dtype=np.float64) - w)) <= 1e-10 * np.max(np.abs(w))


def test_dense_check_on_one_tiny_case():
    """T = 4, d = 2, o = 2, B = 2, non-zero mean: ll_b is log N(y; H mu, H K H^T + R) once sumlogchol_b is replaced by -1/2 log|K^{-1}|,
    and x, Sig, Fmu, Fvar are those of the dense posterior -- everything dense built in 80-bit."""
    d, o, B, T = 2, 2, 2, 4
    cs = np_kf.make_case(d, o, B, T, False, False)
    ref = np_kf.reference(cs)
    for b in range(B):
        P = np_kf.to_dense(cs.Pd[b].astype(LD), cs.Ps[b].astype(LD))
        LP = np_kf.chol(P)
        eye = np.eye(T * d, dtype=LD)
        K = np_kf.solve_upper(LP, np_kf.solve_lower(LP, eye))
        Hb, Rb, Rib = np.zeros((T * o, T * d), dtype=LD), np.zeros((T * o, T * o), dtype=LD), np.zeros((T * o, T * o), dtype=LD)
        yv = np.zeros(T * o, dtype=LD)
        for t in range(T):
            Ri = -2 * cs.nat2[b, t].astype(LD)
            Lr = np_kf.chol(Ri)
            R = np_kf.solve_upper(Lr, np_kf.solve_lower(Lr, np.eye(o, dtype=LD)))
            Hb[t * o:(t + 1) * o, t * d:(t + 1) * d] = cs.H
            Rb[t * o:(t + 1) * o, t * o:(t + 1) * o], Rib[t * o:(t + 1) * o, t * o:(t + 1) * o] = R, Ri
            yv[t * o:(t + 1) * o] = R @ cs.nat1[b, t].astype(LD)
        # the kernels take H mu_p and K^{-1} mu_p as inputs rounded to float64: the dense side takes the same numbers
        hm, plin = cs.Hmu[b].astype(LD).reshape(-1), cs.plin[b].astype(LD).reshape(-1)
        S = Hb @ K @ Hb.T + Rb
        Ls = np_kf.chol(S)
        w = np_kf.solve_lower(Ls, (yv - hm)[:, None])[:, 0]
        logN = -LD(0.5) * T * o * LD(np_kf.LOG2PI) - np.sum(np.log(np.diagonal(Ls))) - LD(0.5) * np.sum(w * w)
        got = ref.ll[b] + cs.sumlogchol[b].astype(LD) + np.sum(np.log(np.diagonal(LP)))
        assert abs(got - logN) <= 1e-16 * ref.all[b], (got, logN)
        Lq = np_kf.chol(P + Hb.T @ Rib @ Hb)
        Sg = np_kf.solve_upper(Lq, np_kf.solve_lower(Lq, eye))
        x = Sg @ (plin + Hb.T @ cs.nat1[b].astype(LD).reshape(-1))
        assert np.max(np.abs(x.reshape(T, d) - ref.x[b])) <= 1e-16 * np.max(np.abs(x))
        for t in range(T):
            blk = Sg[t * d:(t + 1) * d, t * d:(t + 1) * d]
            assert np.max(np.abs(blk - ref.Sig[b, t])) <= 1e-16 * np.max(np.abs(Sg))
            assert np.max(np.abs(cs.H.astype(LD) @ x[t * d:(t + 1) * d] - ref.Fmu[b, t])) <= 1e-16 * np.max(np.abs(ref.Fmu[b]))
            assert np.max(np.abs(np.diagonal(cs.H.astype(LD) @ blk @ cs.H.astype(LD).T) - ref.Fvar[b, t])) <= 1e-16 * np.max(np.abs(ref.Fvar[b]))


@functools.lru_cache(maxsize=None)
def twin_ratios(d, o, case):
    """{output: err / bound} of the reference's own code in float64 against its 80-bit run, on one case of the GPU test."""
    B, T, R0, shared, zero_mean = case
    cs = np_kf.make_case(d, o, B, T, shared, zero_mean)
    ref, tw = np_kf.reference(cs), np_kf.reference(cs, np.float64)
    out = np_kf.local_checks(cs, ref, tw.m0.D, tw.m0.r, tw.m1.r, tw.m0.t1, tw.m0.ldR)
    out.update(np_kf.project_checks(cs, tw.Fmu, tw.Fvar, tw.x, tw.Sig))
    out.update(np_kf.sweep_scalar_checks(cs, ref, tw.logdet, tw.quad, tw.ll, tw.total))
    out.update(np_kf.sweep_array_checks(cs, ref, tw.Sig, tw.x, tw.Fmu, tw.Fvar))
    return out


WORST = {}


def _id(d, o, case):
    B, T, R0, shared, zm = case
    return f"d{d}-o{o}-" + ("long" if T > 10000 else f"B{B}T{T}R{R0}{'s' if shared else ''}{'z' if zm else ''}")


@pytest.mark.parametrize("d,o,case", [pytest.param(d, o, c, id=_id(d, o, c)) for d, o in np_kf.DIMS for c in np_kf.cases_of(d, o)])
def test_float64_twin_holds_the_bounds(d, o, case):
    """Every bound of tests/test_gpu_kf.py holds, with err / bound <= 1, for the reference's own code run in float64, on every case
    that file runs.  (A chain of one node with d = 1 is one scalar equation, cond_2 = 1, and the sweep bound of the array outputs is
    half an ulp there: np_kf.scalar_system gives that case inputs on which fp64 rounds nothing on the way to them.)"""
    ratios = twin_ratios(d, o, case)
    for name, r in ratios.items():
        if r > WORST.get(name, (0.0,))[0]:
            WORST[name] = (r, _id(d, o, case))
    print("\n  " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    print("  largest err / bound of the float64 twin so far: "
          + ", ".join(f"{k} {v[0]:.3f} ({v[1]})" for k, v in sorted(WORST.items())))
    for name, r in ratios.items():
        assert r <= 1.0, (name, d, o, case, r)
