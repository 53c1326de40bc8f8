"""
Host tests (no GPU) of tests/np_cq.py, the 80-bit reference and input generator of tests/test_gpu_cq.py: the reference agrees with the
fp64 oracle within the bound the GPU tests use, the generated precisions are well conditioned, the forced observation nodes are where
the partition says, and the packed-layout helpers invert each other.
"""
import numpy as np
import pytest

from tests import np_cq

DIMS = [1, 3, 8]
# the reference bound of the tolerance rule: the 80-bit and the fp64 elimination of a system with condition number < 20 differ by a
# small multiple of the fp64 rounding unit (condition number x eps x a growth factor of a few: tens of eps); 64 eps is the floor the GPU
# tests grant every output, and the fp64 oracle, the yardstick of those tests, must itself be inside it.  Every check prints its figure
# (measured: 0.1 ... 4.4 eps).
REF_BOUND = 64 * np_cq.EPS


def within(name, got, want, bound=REF_BOUND):
    err = np_cq.rel_err(got, want)
    print(f"  {name}: fp64 oracle against the 80-bit reference {err:.3e} ({err / np_cq.EPS:.1f} eps)")
    assert err <= bound, (name, err)


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("shape", np_cq.SHAPES, ids=lambda s: "B%d-T%d" % s[:2])
def test_reference_posterior_agrees_with_the_fp64_oracle(d, shape):
    st = np_cq.make_state(d, shape)
    ref, orc = np_cq.posterior(st), np_cq.posterior_fp64(st)
    for name in ("x", "Sig", "Sub", "logdet"):
        within(f"d={d} {shape} {name}", getattr(orc, name), getattr(ref, name))
    # the naturals -> SSM route of the oracle gives the same marginals (np_transforms.naturals_to_ssm_params -> marginals)
    from oracle import np_transforms
    lin, diag, sub = (a.astype(np.float64) for a in np_cq.dense_naturals(st))
    q = np_transforms.ssm_from_params(np_transforms.naturals_to_ssm_params(lin[0], diag[0], sub[0]))
    mu, cov = q.marginals
    within(f"d={d} {shape} x through the SSM parameters", mu, ref.x[0])
    within(f"d={d} {shape} Sig through the SSM parameters", cov, ref.Sig[0])


@pytest.mark.parametrize("d", DIMS)
def test_generated_precisions_are_well_conditioned(d):
    shape = np_cq.SHAPES[1]                                      # the smallest one: T = 33
    for kw in (dict(), dict(sites=False), dict(p0=False)):
        st = np_cq.make_state(d, shape, **kw)
        w = np.linalg.eigvalsh(np_cq.precision_dense(st))
        print(f"d={d} {kw}: eigenvalues in [{w[0]:.3f}, {w[-1]:.3f}], condition number {w[-1] / w[0]:.2f}")
        assert w[0] > 0 and w[-1] / w[0] < 20
    for shape in np_cq.SHAPES:
        st = np_cq.make_state(d, shape)
        for b in (0, st.B - 1):
            w = np.linalg.eigvalsh(np_cq.precision_dense(st, b))
            assert w[0] > 0 and w[-1] / w[0] < 20


@pytest.mark.parametrize("shape", np_cq.SHAPES, ids=lambda s: "B%d-T%d" % s[:2])
def test_forced_observation_nodes_follow_the_plan(shape):
    B, T, R0, Rup = shape
    st = np_cq.make_state(3, shape)
    n, R, P, Lpad = st.levels[0]
    assert len(st.levels) >= 2 and n == T and R == R0 and P == -(-T // R) and Lpad % 64 == 0 and Lpad >= B * P
    first_of_segment, last_of_segment = np.arange(P) * R, np.minimum(np.arange(1, P + 1) * R, T) - 1
    for b in range(B):
        obs = set(st.obs_t[b].tolist())
        assert len(obs) == st.obs_t.shape[1]                     # no node twice
        assert {0, 1, 2, T - 1} <= obs
        inner = [p for p in range(P) if 0 < p < P - 1] or [0]
        assert any({first_of_segment[p], last_of_segment[p], last_of_segment[p] - 1} <= obs for p in inner)
        assert any(t >= (P - 1) * R for t in obs)                # the ragged last segment
        assert len(obs) < T                                      # and some node without a site
    assert np_cq.make_state(3, shape, sites=False).obs_t is None and np_cq.make_state(3, shape, p0=False).p0_off is None


def test_packed_layout_helpers():
    shape = np_cq.SHAPES[0]
    st = np_cq.make_state(2, shape)
    lv = st.levels[0]
    flat = np_cq.pack_nodes(st.dyn, lv, np.full(6, 9.0))
    back, mask = np_cq.unpack_nodes(flat, st.B, st.T, 6, lv)
    np.testing.assert_array_equal(back, st.dyn)
    assert mask.sum() == st.dyn.size and np.all(flat[~mask] == 9.0)
    slot = np_cq.slot_array(st, lv)
    assert (slot >= 0).sum() == st.obs_t.size
    # node (b, t) -> ((lane / 64) R + step) 64 + lane % 64 (include/mfgm.h)
    b, j = st.B - 1, 3
    t = st.obs_t[b, j]
    lane = b * lv[2] + t // lv[1]
    assert slot[(lane // 64 * lv[1] + t % lv[1]) * 64 + lane % 64] == b * st.obs_t.shape[1] + j


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("kind", ["dw", "ou"])
def test_reference_kl_and_girsanov_update(d, kind):
    """KL = kl_part + logdet - T d / 2 by construction; theta~ = theta_q - grad KL has no off-diagonal entries away from node 0 (what the
    structured state assumes) and the update is linear in lr; the fp64 oracle's numbers are within the bound of the reference's."""
    shape = np_cq.SHAPES[1]
    st, sd = np_cq.make_state(d, shape), np_cq.sde_inputs(d, kind)
    args = (sd.alpha, sd.beta, sd.qd, sd.dt, sd.init_mu, sd.init_cov)
    ref = np_cq.kl_and_girsanov(st, *args, lr=[0.3, 1.0])
    orc = np_cq.kl_and_girsanov(st, *args, lr=[0.3, 1.0], post=np_cq.posterior_fp64(st))
    print(f"  d={d} {kind}: largest off-diagonal entry of theta_q - grad KL away from node 0: {ref.off_max:.3e}")
    assert ref.off_max < 1e-13                                   # (entries of order one: rounding of the cancellation)
    assert np.all(ref.kl > 0)
    np.testing.assert_allclose(0.3 * ref.dyn_out[1] + 0.7 * st.dyn, ref.dyn_out[0], rtol=0, atol=1e-13 * np.abs(ref.dyn_out[1]).max())
    for name, a, b in zip(("dyn_out lr=0.3", "dyn_out lr=1", "kl", "kl_part"), ref.dyn_out + [ref.kl, ref.kl_part],
                          orc.dyn_out + [orc.kl, orc.kl_part]):
        within(f"d={d} {kind} {name}", b, a)
    # the likelihood side: the 80-bit variational expectations against the oracle's
    from oracle import np_models
    post = np_cq.posterior(st)
    mu, cov = np_cq.at_obs(st, post.x).astype(np.float64), np_cq.at_obs(st, post.Sig).astype(np.float64)
    want = np_models.MultivariateGaussianLik(st.cholR).variational_expectations(mu, cov, st.y).sum(-1)
    within(f"d={d} variational expectations", want, np_cq.ve_compact(mu, cov, st.y, st.cholR))
