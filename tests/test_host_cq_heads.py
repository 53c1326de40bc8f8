"""
Host tests (no GPU) of tests/np_cq_heads.py: the level-0 reduce with the observed nodes eliminated last gives the five blocks of the
sequential reduce, the separator system either of them leaves has the marginals of the whole-chain elimination of tests/np_cq.py at
the separator nodes, and the generated states are what tests/test_gpu_cq_heads.py says they are.

Bounds.  Both reduces are eliminations of a system with condition number < 20 (tests/test_host_cq.py), so two of them in one
precision differ by a small multiple of condition number x rounding unit: the 80-bit pair is held to 20 x 64 longdouble units, an
fp64 result to max(8 x yardstick, 64 eps) of the 80-bit one -- the rule of tests/test_gpu_cq.py -- with the fp64 sequential reduce as
the yardstick.  Every check prints its figure.
"""
import functools

import numpy as np
import pytest

from tests import np_cq
from tests import np_cq_heads as nh

LD_BOUND = 20 * 64 * float(np.finfo(np_cq.LD).eps)
FLOOR = 64 * np_cq.EPS
BLOCKS = ("Dhat", "rhat", "S", "Rsub", "rho")
CASES = [(d, s) for s in nh.SHAPES for d in nh.DIMS]
IDS = [f"{i}-d{d}" for i in nh.SHAPE_IDS for d in nh.DIMS]


@functools.lru_cache(maxsize=None)
def reduces(d, shape):
    st = nh.make_state(d, shape)
    return st, nh.reduce_sequential(st, np_cq.LD), nh.reduce_heads_last(st, st.q, np_cq.LD)


@pytest.mark.parametrize("d,shape", CASES, ids=IDS)
def test_heads_last_gives_the_sequential_blocks(d, shape):
    st, seq, hl = reduces(d, shape)
    seq64, hl64 = nh.reduce_sequential(st, np.float64), nh.reduce_heads_last(st, st.q, np.float64)
    for name in BLOCKS:
        e80 = np_cq.rel_err(hl[name], seq[name])
        yard, e64 = np_cq.rel_err(seq64[name], seq[name]), np_cq.rel_err(hl64[name], seq[name])
        print(f"  {name}: 80-bit heads-last against 80-bit sequential {e80:.3e}; fp64 heads-last {e64:.3e}, fp64 sequential (yardstick) {yard:.3e}")
        assert hl64[name].dtype == np.float64
        assert e80 <= LD_BOUND, (name, e80)
        assert e64 <= max(8.0 * yard, FLOOR), (name, e64, yard)
    # separator 0 has nothing to its left; the spike and the corrections of segment 0 are zero
    for name in ("S", "Rsub", "rho"):
        assert not np.any(hl[name][:, 0])


@pytest.mark.parametrize("d,shape", CASES, ids=IDS)
def test_separator_system_has_the_marginals_of_the_whole_chain(d, shape):
    st, seq, hl = reduces(d, shape)
    ref = np_cq.posterior(st)
    for what, red in (("sequential", seq), ("heads-last", hl)):
        nodes, x, Sig = nh.separator_posterior(st, red)
        for name, got, want in (("x", x, ref.x[:, nodes]), ("Sig", Sig, ref.Sig[:, nodes])):
            err = np_cq.rel_err(got, want)
            print(f"  {what} {name} at the separators against np_cq.posterior: {err:.3e}")
            assert err <= LD_BOUND, (what, name, err)


@pytest.mark.parametrize("shape", nh.SHAPES, ids=nh.SHAPE_IDS)
def test_generated_states(shape):
    B, T, R0, Rup, q = shape
    st = nh.make_state(3, shape)
    n, R, P, Lpad = st.levels[0]
    assert n == T and R % q == 0 and R == R0
    obs = st.obs_t
    assert obs.shape[0] == B and np.all(obs % q == 0) and np.all((obs % R) % q == 0)
    assert all(len(set(row)) == obs.shape[1] for row in obs)
    last_head = (T - 1) // q * q
    assert np.all((obs == last_head).any(axis=1))
    if B > 1 and shape != nh.SHAPES[-1]:
        assert (obs == 0).any(axis=1).sum() == B - 1                # one chain starts on an unobserved head
        assert len({tuple(sorted(row)) for row in obs}) > 1         # the chains observe different heads
    else:
        assert np.all((obs == 0).any(axis=1))
    if shape == nh.SHAPES[-1]:
        assert obs.shape[1] == len(range(0, T, q))
    else:
        assert obs.shape[1] < len(range(0, T, q))                   # some heads carry no observation
    # what each shape is there for
    last_len = T - (P - 1) * R
    if shape == nh.SHAPES[0]:
        assert R // q == 2 and last_len == 1 and (T - 1) % q == 0
    if shape == nh.SHAPES[1]:
        assert R // q == 3 and (last_len - 1) % q == 2              # the last node follows a one-node interior
    if shape == nh.SHAPES[2]:
        assert Lpad // 64 == 4 and B * P < Lpad and q == 2 and P == 3
    if shape == nh.SHAPES[3]:
        assert R == q
    if shape == nh.SHAPES[4]:
        assert T % R == 0
    w = np.linalg.eigvalsh(np_cq.precision_dense(st))
    assert w[0] > 0 and w[-1] / w[0] < 20
