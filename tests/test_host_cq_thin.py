"""CPU tests of the thinned cq pair route: the store rule, the host restatement "kept records + one forward step" (tests/np_cq_thin.py)
against the full forward recursion on the states the GPU tests use, and the Python-side routing of the `thin` marker (no GPU: the
library is replaced by a recorder)."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from tests import np_cq
from tests import np_cq_heads as nh
from tests import np_cq_thin as nt


# ---- the store rule -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 3, 4, 9, 15, 16, 100])
def test_kept_set(R):
    k = [s for s in range(R) if nt.kept(s, R)]
    assert k == sorted(set(range(0, R, 2)) | {R - 1})
    assert 0 in k and R - 1 in k                         # node 0 of a chain (p0_off) and the record the right neighbour reads
    # a record that is not kept has a kept one right before it, in the same segment
    assert all(nt.kept(s - 1, R) and s >= 1 for s in range(R) if not nt.kept(s, R))


def test_stored_fraction():
    assert nt.stored_fraction(100 * 7, 100) == 0.51      # R even: R / 2 even steps and step R - 1
    assert nt.stored_fraction(9 * 5, 9) == 5 / 9         # R odd: step R - 1 is an even one
    assert nt.stored_fraction(15 * 2, 15) == 8 / 15
    # a short last segment: its steps follow the same rule on their local index (its last node need not be kept: no sweep reads it)
    m = nt.kept_nodes(257, 8)
    assert m[256] and m.sum() == 32 * 5 + 1
    m = nt.kept_nodes(47, 15)
    assert list(np.flatnonzero(~m[45:])) == [1] and m[44]
    m = nt.kept_nodes(36, 16)                            # last segment of four nodes: local steps 0 and 2
    assert list(np.flatnonzero(m[32:])) == [0, 2]


# ---- kept records + one forward step = the full recursion ----------------------------------------------------------------------------------
STATES = [("heads", d, s) for s in nh.SHAPES[:2] + [(3, 100, 9, 3, 3), (2, 47, 15, 3, 5)] for d in (1, 3, 6)] + \
         [("plain", d, s) for s in np_cq.SHAPES[:2] for d in (2, 6)]


def _state(kind, d, shape):
    return nh.make_state(d, shape) if kind == "heads" else np_cq.make_state(d, shape)


@pytest.mark.parametrize("kind,d,shape", STATES, ids=[f"{k}-d{d}-{'x'.join(map(str, s))}" for k, d, s in STATES])
def test_rebuilt_records_reproduce_the_forward_recursion(kind, d, shape):
    st = _state(kind, d, shape)
    R = st.levels[0][1]
    keep = nt.kept_nodes(st.T, R)
    if st.obs_t is not None and kind == "plain":
        assert np.any(~keep[st.obs_t])                   # a site on a rebuilt node is covered
    post = np_cq.posterior(st)
    for dtype in (np.float64, np_cq.LD):
        P, z, logdet = nt.forward_records(st, dtype)
        # the recursion is np_cq's: same log-determinant, and P_{T-1} is the last node's marginal covariance, z_{T-1} its mean
        eps = float(np.finfo(dtype).eps)
        assert np_cq.rel_err(logdet, post.logdet) <= 64 * max(eps, float(np.finfo(np_cq.LD).eps)) * st.T
        assert np_cq.rel_err(P[:, -1], post.Sig[:, -1]) <= 1e3 * max(eps, float(np.finfo(np_cq.LD).eps))
        assert np_cq.rel_err(z[:, -1], post.x[:, -1]) <= 1e3 * max(eps, float(np.finfo(np_cq.LD).eps))
        Pr, zr = nt.rebuilt_records(st, R, (P, z), dtype)
        assert np.all(np.isfinite(Pr)) and np.all(np.isfinite(zr))     # no unkept record was read
        # the same calls on the same inputs: the rebuilt records ARE the recursion's
        np.testing.assert_array_equal(Pr, P)
        np.testing.assert_array_equal(zr, z)
    # ... and np_cq's OWN: record t is the last node's marginal of the chain cut after node t, which np_cq.posterior derives in
    # Cholesky form with a forward and a backward pass.  Rebuilt nodes: the first, one in the middle, the last, every observed one
    # (up to four), in the first and the last chain; the bound is that of the checks above
    ld_eps = float(np.finfo(np_cq.LD).eps)
    rebuilt = np.flatnonzero(~keep)
    picks = {int(rebuilt[0]), int(rebuilt[len(rebuilt) // 2]), int(rebuilt[-1])}
    for b in sorted({0, st.B - 1}):
        obs = [] if st.obs_t is None else [int(t) for t in st.obs_t[b] if not keep[t]][:4]
        for t in sorted(picks | set(obs)):
            cut = np_cq.posterior(nt.truncated(st, b, t))
            for dtype in (np.float64, np_cq.LD):
                P, z, _ = nt.forward_records(st, dtype)
                Pr, zr = nt.rebuilt_records(st, R, (P, z), dtype)
                bound = 1e3 * max(float(np.finfo(dtype).eps), ld_eps)
                assert np_cq.rel_err(Pr[b, t], cut.Sig[0, -1]) <= bound, (b, t, dtype)
                assert np_cq.rel_err(zr[b, t], cut.x[0, -1]) <= bound, (b, t, dtype)


# ---- the marker's routing --------------------------------------------------------------------------------------------------------------------
class _Struct(ctypes.Structure):
    _fields_ = [("site_lin", ctypes.c_void_p), ("site_sym", ctypes.c_void_p)]


class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append(name)
            return 0
        return fn


@pytest.fixture
def fake_plan(monkeypatch):
    import torch
    import vidp_amd
    from vidp_amd import packed
    monkeypatch.setattr(packed, "_stream", lambda: ctypes.c_void_p(0))
    plan = object.__new__(packed.Plan)
    plan.lib, plan.h, plan.B, plan.device, plan.ws, plan.info, plan.epoch = _Recorder(), None, 2, "cpu", None, None, 0
    t = lambda: torch.zeros(4, dtype=torch.float64)
    cq = SimpleNamespace(struct=lambda: _Struct())
    return vidp_amd, plan, cq, t


def test_marker_routing(fake_plan):
    _, plan, cq, t = fake_plan
    bufs = [dict(L=t(), y=t()), dict(L=t(), y=t())]
    for thin, stride, entry in ((True, None, "mfgm_cq_factor_pair_thin"), (False, None, "mfgm_cq_factor_pair"),
                                (False, 4, "mfgm_cq_factor_pair_heads"), (True, 4, "mfgm_cq_factor_pair_thin")):
        plan.lib.calls.clear()
        plan._heads_buf = (4, t())
        f, f2 = plan.cq_factor_pair(cq, (t(), t()), out=bufs[0], out2=bufs[1], head_stride=stride, thin=thin)
        assert plan.lib.calls == [entry]
        # a thinned first factor carries the marker, a full factor's dict holds arrays only; the buffer dicts always say which
        assert (f.get("thin", False), "thin" in f2, bufs[0]["thin"], bufs[1]["thin"]) == (thin, False, thin, False)
        assert ("thin" in f) == thin
        plan.lib.calls.clear()
        s = plan.cq_selinv_kl(cq, f["L"], f["y"], ctypes.c_int(0), want_marginals=False, only_level=0, thin=f.get("thin", False))
        assert plan.lib.calls == ["mfgm_cq_selinv_kl_thin" if thin else "mfgm_cq_selinv_kl"] and s["x"] is None
    # a plain factorisation into a buffer that held a thinned factor resets the buffer's marker (its own result is tensors only)
    for kw in ({}, dict(use_ahead=True)):
        bufs[0]["thin"] = True
        f = plan.cq_factor(cq, out=bufs[0], **kw)
        assert sorted(f) == ["L", "logdet", "y"] and bufs[0]["thin"] is False
    # the Girsanov sweep has no form that reads a thinned factor: refused before anything is launched
    plan.lib.calls.clear()
    with pytest.raises(ValueError, match="thinned"):
        plan.cq_selinv_girsanov(cq, t(), t(), None, t(), only_level=0, alt=True, thin=True)
    assert plan.lib.calls == []

