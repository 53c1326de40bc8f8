"""
Pins tests/np_quad.py -- the reference the GPU quadrature tests (tests/test_gpu_quad.py) compare the HIP kernels with -- on the CPU:
against the oracle's closed forms at d = 3 (a degree-6 polynomial is exact under both), against the oracle's restatement of the
reference quadrature at d <= 2, its autograd gradients against fourth-order difference quotients, and its own float64 rounding
(the same gradients with the nodes visited in reverse order).
"""
import numpy as np

from oracle import np_sde
from tests import np_quad
from tests.helpers import QUAD_KL_CASES, assert_close, quad_kl_case, random_quad_path


def _expectations(mu, cov, sub):
    return mu, cov + mu[:, :, None] * mu[:, None, :], sub + mu[1:, :, None] * mu[:-1, None, :]


def _spd(rng, d, lo=0.5):
    M = 0.3 * rng.normal(size=(d, d))
    return M @ M.T + lo * np.eye(d)


def test_closed_forms_at_d3(rng):
    """d = 3, kind 12 (double well), diagonal q: kl, esde and linearize agree with the oracle's closed forms to 1e-11 relative."""
    d, T, dt = 3, 5, 0.05
    mu, cov, sub = (x[0] for x in random_quad_path(rng, 1, T, d))
    qd = 0.5 + rng.random(d)
    sde = np_sde.DoubleWellSDE(np.diag(qd), scale=2.0, c=0.7)
    th = list(np_sde.drift_cubic(sde))
    init_mu, init_cov = 0.1 * rng.normal(size=d), _spd(rng, d)
    al, be = sde.cubic(dt)
    want, (w1, wd, ws) = np_sde.sde_ssm_kl_closed_form(mu, cov, sub, al, be, qd, dt, init_mu, init_cov)
    got = np_quad.kl(12, th, dt, np.diag(qd), init_mu, init_cov, mu[None], cov[None], sub[None])
    np.testing.assert_allclose(got["kl"][0], want, rtol=1e-11)
    assert got["abs"][0] >= abs(want)
    for a, b in ((got["g1"][0], w1), (got["gd"][0], wd), (got["gs"][0], ws)):
        assert_close(a, b, rtol=1e-10, scale_atol=1e-11)
    # E_sde: the closed form takes the linear drift's own parameters (f_L = A x + b; the kernels' is -A x + b) and carries dt
    A, b = 0.5 * rng.normal(size=(T, d, d)), rng.normal(size=(T, d))
    E, dm, dS, _, _, _ = np_quad.esde(12, th, np.diag(qd), mu, cov, A, b)
    wE, wm, wS = np_sde.e_sde_closed_form(th[0], th[1], qd, -A, b, mu, cov, 1.0)
    np.testing.assert_allclose(E.sum(), wE, rtol=1e-11)
    assert_close(dm, wm, rtol=1e-10, scale_atol=1e-11)
    assert_close(dS, wS, rtol=1e-10, scale_atol=1e-11)
    lin = np_sde.linearize_sde(sde, np.arange(T + 1) * dt, mu, cov, init_mu, init_cov, closed_form=True)
    gA, gb, aA, ab = np_quad.linearize(12, th, dt, mu, cov)
    np.testing.assert_allclose(gA, lin.A, rtol=1e-11)            # (the off-diagonals are zeros in both)
    # b = dt (E f - E[J] m) is a difference of two terms: 1e-11 of their absolute sum where they cancel
    assert np.all(np.abs(gb - lin.b) <= 1e-11 * np.maximum(np.abs(lin.b), ab))
    assert np.all(aA >= np.abs(gA) - 1e-15) and np.all(ab >= np.abs(gb) - 1e-15)


def test_kl_against_the_oracle_quadrature(rng):
    """d <= 2: Van der Pol with a full q, and the ReLU network drift, against np_sde.sde_ssm_kl_from_expectations at 1e-10."""
    dt = 0.05
    for kind in (10, 11):
        d, T = (2, 5) if kind == 10 else (1, 6)
        mu, cov, sub = (x[0] for x in random_quad_path(rng, 1, T, d))
        init_mu, init_cov = 0.1 * rng.normal(size=d), _spd(rng, d)
        if kind == 10:
            q = np.array([[0.5, 0.12], [0.12, 0.4]])
            sde, th, nh = np_sde.VanderPolSDE(1.3, 0.9, q), [1.3, 0.9], 0
        else:
            q = np.array([[0.7]])
            w = (rng.normal(size=(1, 3)), 0.1 * rng.normal(size=3), rng.normal(size=(3, 1)), np.array([0.2]))
            sde, th, nh = np_sde.MLPDriftSDE(w, q), np.concatenate([x.reshape(-1) for x in w]), 3
        want = np_sde.sde_ssm_kl_from_expectations(*_expectations(mu, cov, sub), sde, dt, init_mu, init_cov)
        got = np_quad.kl(kind, th, dt, q, init_mu, init_cov, mu[None], cov[None], sub[None], nh=nh, grad=False)
        np.testing.assert_allclose(got["kl"][0], want, rtol=1e-10)


def test_autograd_gradients_against_difference_quotients(rng):
    """d = 3, kind 12, full q: np_quad's autograd gradients against np_sde.sde_ssm_kl_grads_fd(richardson=True) at the tolerance
    tests/test_gpu_api.py::test_cvi_sites_sde_coupled_drifts uses for that quotient (1e-8 relative, floor 1e-6 of the scale)."""
    d, T, dt = 3, 4, 0.05
    mu, cov, sub = (x[0] for x in random_quad_path(rng, 1, T, d))
    q = np.array([[0.8, -0.2, 0.1], [-0.2, 0.6, 0.15], [0.1, 0.15, 0.7]])
    sde = np_sde.DoubleWellSDE(q, scale=2.0, c=0.7)
    init_mu, init_cov = 0.1 * rng.normal(size=d), _spd(rng, d)
    got = np_quad.kl(12, list(np_sde.drift_cubic(sde)), dt, q, init_mu, init_cov, mu[None], cov[None], sub[None])
    want = np_sde.sde_ssm_kl_grads_fd(*_expectations(mu, cov, sub), sde, dt, init_mu, init_cov, eps=2e-4, richardson=True)
    for a, b in zip((got["g1"][0], got["gd"][0], got["gs"][0]), want):
        assert_close(a, b, rtol=1e-8, scale_atol=1e-6)
    # the drift-parameter gradient against a fourth-order quotient of np_quad's own value
    th0 = np.array(np_sde.drift_cubic(sde))
    val = lambda th: np_quad.kl(12, th, dt, q, init_mu, init_cov, mu[None], cov[None], sub[None], grad=False)["kl"][0]
    for p in range(2):
        e = np.zeros(2); e[p] = 1e-3
        fd = (8 * (val(th0 + e) - val(th0 - e)) - (val(th0 + 2 * e) - val(th0 - 2 * e))) / 12e-3
        np.testing.assert_allclose(got["gth"][0][p], fd, rtol=1e-8)


def reversed_order_self_difference(c):
    """max |g - g_reversed| / max |g| per gradient array (g1, gd, gs, gth) of np_quad.kl: the reference's own float64 rounding."""
    args = (c["kind"], c["th"], c["dt"], c["q"], c["mu0"], c["P0"], c["mu"], c["cov"], c["sub"])
    a, b = np_quad.kl(*args, nh=c["nh"]), np_quad.kl(*args, nh=c["nh"], reverse=True)
    return {k: float(np.max(np.abs(a[k] - b[k])) / np.max(np.abs(a[k]))) for k in ("g1", "gd", "gs", "gth")}


def test_gradients_do_not_depend_on_the_node_order():
    """np_quad.kl's autograd gradients with the nodes visited in reverse order, on every case of the GPU parity test (kinds 10 .. 15 with
    that test's own inputs and parameters, tests/helpers.quad_kl_case): the difference is float64 rounding.  The GPU test may loosen
    its gradient tolerance for a case only if this figure exceeds a tenth of its floor, 1e-11 of the array's largest magnitude; it
    does for none (largest figure: 2.4e-13, g1 of kinds 10 and 15), so every case keeps the project's tolerance."""
    for kind in sorted(QUAD_KL_CASES):
        fig = reversed_order_self_difference(quad_kl_case(kind))
        print(f"np_quad.kl kind {kind}: reversed-order self-difference / max|g| " + " ".join(f"{k} {v:.2e}" for k, v in fig.items()))
        assert max(fig.values()) < 1e-11
