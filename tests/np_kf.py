"""
Host reference of the fused Kalman filter with sites (csrc/mfgm_kf.h, the mfgm_kf_sites_* entry points of csrc/mfgm_api_sweeps.hip): a
plain restatement of the operation in np.longdouble (80-bit on x86: eps 1.08e-19), which takes the dtype as an argument so that the
same code also runs in float64 as its own twin (tests/test_host_kf.py).  No GPU, no torch.

Every output comes with the sum of the absolute values of its terms, which the bounds of tests/test_gpu_kf.py are taken relative to.
The block Cholesky, the forward solve and the selected inverse are one sequential pass over the nodes (batched over the chains); the
per-node terms are whole-array expressions, so that T = 16385 costs a loop of d x d steps and nothing else.
"""
from types import SimpleNamespace

import numpy as np

from tests.helpers import random_dominant_btd

LD = np.longdouble
EPS = 2.0 ** -52
LOG2PI = 1.8378770664093454835606594728112353
SITE_SCALE = 0.05          # size of the site precisions next to the prior's (make_case)
SPREAD = 12.0              # largest coordinate scale of the prior precision (make_case)


# ---- small dense algebra in any dtype (numpy.linalg has no long double) ------------------------------------------------------------
def _T(x):
    return np.swapaxes(x, -1, -2)


def chol(A):
    """Lower Cholesky factor of [..., d, d] (the lower triangle is read); NaN where a pivot is not positive."""
    d = A.shape[-1]
    L = np.zeros_like(A)
    for j in range(d):
        s = A[..., j, j] - np.sum(L[..., j, :j] * L[..., j, :j], axis=-1)
        with np.errstate(invalid="ignore"):
            L[..., j, j] = np.sqrt(s)
        if j + 1 < d:
            L[..., j + 1:, j] = (A[..., j + 1:, j] - np.einsum("...ik,...k->...i", L[..., j + 1:, :j], L[..., j, :j])) / L[..., j, j, None]
    return L


def solve_lower(L, Bm):
    """L^{-1} Bm, Bm [..., d, k]."""
    d = L.shape[-1]
    X = np.zeros(np.broadcast_shapes(L.shape[:-2], Bm.shape[:-2]) + Bm.shape[-2:], dtype=L.dtype)
    for i in range(d):
        X[..., i, :] = (Bm[..., i, :] - np.einsum("...k,...kj->...j", L[..., i, :i], X[..., :i, :])) / L[..., i, i, None]
    return X


def solve_upper(L, Bm):
    """L^{-T} Bm."""
    d = L.shape[-1]
    X = np.zeros(np.broadcast_shapes(L.shape[:-2], Bm.shape[:-2]) + Bm.shape[-2:], dtype=L.dtype)
    for i in range(d - 1, -1, -1):
        X[..., i, :] = (Bm[..., i, :] - np.einsum("...k,...kj->...j", L[..., i + 1:, i], X[..., i + 1:, :])) / L[..., i, i, None]
    return X


def to_dense(diag, sub):
    """[T, d, d], [T - 1, d, d] (block (t + 1, t)) -> symmetric dense [T d, T d]."""
    T, d = diag.shape[0], diag.shape[-1]
    out = np.zeros((T * d, T * d), dtype=diag.dtype)
    for k in range(T):
        out[k * d:(k + 1) * d, k * d:(k + 1) * d] = diag[k]
    for k in range(T - 1):
        out[(k + 1) * d:(k + 2) * d, k * d:(k + 1) * d] = sub[k]
        out[k * d:(k + 1) * d, (k + 1) * d:(k + 2) * d] = sub[k].T
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def make_H(d, o):
    """Emission matrix [o, d]: every entry nonzero, all distinct, the two rows no multiples of each other (d >= 2; at d = 1 any two
    rows are, and the entries are short binary fractions, which scalar_system needs)."""
    i = np.arange(d)
    rows = [0.7 + 0.11 * i, (-1.0) ** i * (0.35 + 0.09 * i)] if d > 1 else [np.array([0.75]), np.array([0.375])]
    H = np.stack(rows[:o])
    assert np.all(H != 0) and len(set(H.reshape(-1).tolist())) == H.size
    if o == 2 and d > 1:
        assert np.linalg.matrix_rank(H) == 2
    return H


def sites_for(rng, Bs, T, o):
    """nat1 [Bs, T, o] and nat2 [Bs, T, o, o]: R^{-1} = -2 nat2 with eigenvalues within SITE_SCALE [0.5, 4.5]; for o = 2 symmetric negative definite
    to the bit with an off-diagonal that is nonzero and changes size and sign with t."""
    nat1 = rng.normal(size=(Bs, T, o))
    if o == 1:
        return nat1, -SITE_SCALE * (0.25 + 1.25 * rng.random(size=(Bs, T, 1, 1)))
    a, b = SITE_SCALE * (1.0 + 2.0 * rng.random(size=(Bs, T))), SITE_SCALE * (1.0 + 2.0 * rng.random(size=(Bs, T)))
    s = (0.3 + 0.7 * rng.random(size=(Bs, T))) * np.where((np.arange(T) % 3 == 1)[None, :], -1.0, 1.0)
    c = 0.45 * np.sqrt(a * b) * s
    Ri = np.stack([np.stack([a, c], -1), np.stack([c, b], -1)], -2)
    return nat1, -0.5 * Ri


def scalar_system(H, o, B, Bs, zero_mean):
    """d = 1, T = 1: the posterior precision is one number and cond_2 = 1, so the sweep bound 0.5 EPS cond_2 max|want| of Sig, x, Fmu
    and Fvar is half an ulp, which no fp64 route through a square root and two divisions holds on general inputs.  It can be held only
    where that route rounds nothing, so here every input is a short binary fraction and the prior precision is chosen so that
    D = Pd + h R^{-1} h is 4, 16 or 64 exactly: L, y, x, Sig, Fmu and Fvar are then exact in fp64 in any order of operations, and any
    mapping mistake still shows in full.  The chains (and the sites, when not shared) all differ.  Returns Pd [B, 1, 1, 1], mu_p
    [B, 1, 1] or None, nat1 [Bs, 1, o], nat2 [Bs, 1, o, o]."""
    k = np.arange(Bs, dtype=np.float64)
    nat1 = np.stack([0.5 + 0.25 * k, -0.75 + 0.125 * k][:o], -1)[:, None, :]
    if o == 1:
        Ri = (0.125 * (1.0 + k))[:, None, None, None]
    else:
        a, b, c = 0.125 * (1.0 + k), 0.25 + 0.0 * k, 0.0625 * (-1.0) ** k
        Ri = np.stack([np.stack([a, c], -1), np.stack([c, b], -1)], -2)[:, None]
    hrh = np.einsum("ai,btac,cj->btij", H, np.broadcast_to(Ri, (B, 1, o, o)), H)
    Pd = (4.0 ** (1 + np.arange(B) % 3))[:, None, None, None] - hrh
    assert np.all(Pd > 0) and np.all(np.log2(Pd + hrh) % 2 == 0)
    mu_p = None if zero_mean else (0.5 - 0.75 * np.arange(B, dtype=np.float64))[:, None, None]
    return Pd, mu_p, nat1, -0.5 * Ri


def cond_of(cs, window=64):
    """cond_2 of the dense posterior precision of every chain [B]; beyond 128 nodes the largest over dense windows of `window` nodes
    (every half window)."""
    ref = assemble(cs, 0, np.float64)
    D = np.asarray(ref.D, dtype=np.float64)
    out = np.empty(cs.B)
    for b in range(cs.B):
        if cs.T <= 2 * window:
            out[b] = np.linalg.cond(to_dense(D[b], cs.Ps[b] if cs.T > 1 else None))
        else:
            starts = list(range(0, cs.T - window, window // 2)) + [cs.T - window]
            out[b] = max(np.linalg.cond(to_dense(D[b, s:s + window], cs.Ps[b, s:s + window - 1])) for s in starts)
    return out


def make_case(d, o, B, T, shared_sites, zero_mean, prior=None, seed=0):
    """Seeded inputs of one problem in which no mapping mistake cancels: H of make_H; a prior precision (Pd [B, T, d, d], Ps
    [B, T - 1, d, d] = the blocks (t + 1, t)) that is block-tri-diagonal, SPD, another for every chain and whose sub-diagonal blocks are
    not symmetric (tests.helpers.random_dominant_btd; `prior` = (Pd, Ps, mu_p or None, sumlogchol) replaces it); sites of sites_for,
    [1, T, ...] when shared (the chains then still differ through the prior and Hmu); a prior mean mu_p [B, T, d] with Hmu = H mu_p
    and plin = K^{-1} mu_p, both rounded to float64 (inputs as the kernels get them) or, with zero_mean, absent; sumlogchol [B] and cst
    as the log-likelihood takes them.  Asserts cond_2 <= 1e4 of the dense posterior precision (kept as cs.cond [B]) and, for o = 2,
    (|ad| + |bc|) / |ad - bc| <= 4 at every site."""
    rng = np.random.default_rng([7411, d, o, B, T, int(shared_sites), int(zero_mean), seed])
    H = make_H(d, o)
    if prior is None:
        Pd, Ps = random_dominant_btd(rng, (B,), T, d)
        # P -> S P S with S = diag(s), s over [1, SPREAD] and another for every chain, node and coordinate: still SPD and
        # block-tri-diagonal, and cond_2 in the hundreds to thousands, which is what the sweep bound 0.5 EPS cond_2 is made for
        s = np.stack([rng.permutation(SPREAD ** np.linspace(0.0, 1.0, T * d)).reshape(T, d) for _ in range(B)])
        Pd = s[..., :, None] * Pd * s[..., None, :]
        if T > 1:
            Ps = s[:, 1:, :, None] * Ps * s[:, :-1, None, :]
        mu_p = None if zero_mean else rng.normal(size=(B, T, d))
        slc = rng.normal(size=B) * T
    else:
        Pd, Ps, mu_p, slc = prior
    Bs = 1 if shared_sites else B
    nat1, nat2 = sites_for(rng, Bs, T, o)
    if prior is None and d == 1 and T == 1:
        Pd, mu_p, nat1, nat2 = scalar_system(H, o, B, Bs, zero_mean)
    Pd = 0.5 * (Pd + _T(Pd))
    if Ps is None:
        Ps = np.zeros((B, 0, d, d))
    if d > 1 and T > 1:
        assert not np.array_equal(Ps, _T(Ps))
    assert np.array_equal(nat2, _T(nat2))
    cs = SimpleNamespace(d=d, o=o, B=B, T=T, Bs=Bs, H=H, Pd=Pd, Ps=Ps, nat1=nat1, nat2=nat2, mu_p=mu_p, Hmu=None, plin=None,
                         sumlogchol=np.asarray(slc, dtype=np.float64), cst=-0.5 * LOG2PI * o * T)
    if mu_p is not None:
        m = mu_p.astype(LD)
        cs.Hmu = np.einsum("ai,bti->bta", H.astype(LD), m).astype(np.float64)
        pl = np.einsum("btij,btj->bti", Pd.astype(LD), m)
        if T > 1:
            S = Ps.astype(LD)
            pl[:, 1:] += np.einsum("btij,btj->bti", S, m[:, :-1])
            pl[:, :-1] += np.einsum("btji,btj->bti", S, m[:, 1:])
        cs.plin = pl.astype(np.float64)
    if o == 2:
        Ri = -2.0 * nat2
        k2 = (np.abs(Ri[..., 0, 0] * Ri[..., 1, 1]) + np.abs(Ri[..., 0, 1] * Ri[..., 1, 0])) / np.abs(
            Ri[..., 0, 0] * Ri[..., 1, 1] - Ri[..., 0, 1] * Ri[..., 1, 0])
        assert k2.max() <= 4.0, k2.max()
    cs.cond = cond_of(cs)
    assert cs.cond.max() <= 1e4, cs.cond.max()
    for a in (cs.H, cs.Pd, cs.Ps, cs.nat1, cs.nat2, cs.sumlogchol, cs.cond) + tuple(x for x in (cs.mu_p, cs.Hmu, cs.plin) if x is not None):
        a.setflags(write=False)
    return cs


# ---- the operation -----------------------------------------------------------------------------------------------------------------------
def assemble(cs, mode, dt=LD):
    """k_kf_assemble: D_t = Pd_t + H^T R_t^{-1} H [B, T, d, d]; r_t = H^T (nat1 - R^{-1} H mu_p) (mode 0) or plin + H^T nat1 (mode 1)
    [B, T, d]; per chain t1 = sum_t (y - H mu_p)^T R^{-1} (y - H mu_p) and ldR = sum_t log det R_t^{-1} with R^{-1} = -2 nat2,
    y = R nat1 -- each with the sum of its absolute terms (aD, ar, at1, aldR).  For o = 2 the absolute terms of y carry the condition
    (|ad| + |bc|) / |det| of the 2 x 2 solve; a term of ldR has the scale 1 + |log det|."""
    o, B, T = cs.o, cs.B, cs.T
    H = cs.H.astype(dt)
    n1 = np.broadcast_to(cs.nat1.astype(dt), (B, T, o))
    Ri = np.broadcast_to(dt(-2.0) * cs.nat2.astype(dt), (B, T, o, o))
    hm = np.zeros((B, T, o), dtype=dt) if cs.Hmu is None else cs.Hmu.astype(dt)
    Pd = cs.Pd.astype(dt)
    D, aD = Pd.copy(), np.abs(Pd)
    for a in range(o):
        for c in range(o):
            term = H[a][None, None, :, None] * Ri[:, :, a, c, None, None] * H[c][None, None, None, :]
            D, aD = D + term, aD + np.abs(term)
    if o == 1:
        y = n1 / Ri[..., 0]
        ay = np.abs(y)
        det = Ri[..., 0, 0]
    else:
        p, q = Ri[..., 0, 0] * Ri[..., 1, 1], Ri[..., 0, 1] * Ri[..., 1, 0]
        det = p - q
        kap = (np.abs(p) + np.abs(q)) / np.abs(det)
        y = np.stack([(Ri[..., 1, 1] * n1[..., 0] - Ri[..., 0, 1] * n1[..., 1]) / det,
                      (Ri[..., 0, 0] * n1[..., 1] - Ri[..., 1, 0] * n1[..., 0]) / det], -1)
        ay = np.stack([(np.abs(Ri[..., 1, 1] * n1[..., 0]) + np.abs(Ri[..., 0, 1] * n1[..., 1])) / np.abs(det),
                       (np.abs(Ri[..., 0, 0] * n1[..., 1]) + np.abs(Ri[..., 1, 0] * n1[..., 0])) / np.abs(det)], -1) * kap[..., None]
    v0, av0 = n1.copy(), np.abs(n1)                    # R^{-1} (y - H mu_p) = nat1 - R^{-1} H mu_p
    for c in range(o):
        term = Ri[..., :, c] * hm[..., None, c]
        v0, av0 = v0 - term, av0 + np.abs(term)
    v, av = (v0, av0) if mode == 0 else (n1, np.abs(n1))
    if mode == 1 and cs.plin is not None:
        r = cs.plin.astype(dt).copy()
    else:
        r = np.zeros((B, T, cs.d), dtype=dt)
    ar = np.abs(r)
    for a in range(o):
        term = H[a][None, None, :] * v[..., a, None]
        r, ar = r + term, ar + np.abs(H[a])[None, None, :] * av[..., a, None]
    t1 = np.sum(np.sum((y - hm) * v0, axis=-1), axis=-1)
    at1 = np.sum(np.sum((ay + np.abs(hm)) * av0, axis=-1), axis=-1)
    ld = np.log(det)
    return SimpleNamespace(D=D, aD=aD, r=r, ar=ar, t1=t1, at1=at1, ldR=np.sum(ld, axis=-1), aldR=np.sum(1.0 + np.abs(ld), axis=-1))


def factor(D, Ps, dt=LD):
    """Sequential block Cholesky of the block-tri-diagonal (D, Ps): L [B, T, d, d], G [B, T - 1, d, d] = the blocks (t + 1, t),
    log|L| [B] = sum log L_ii and the sum of |log L_ii|."""
    B, T, d = D.shape[:3]
    S = Ps.astype(dt)
    L, G = np.zeros((B, T, d, d), dtype=dt), np.zeros((B, max(T - 1, 0), d, d), dtype=dt)
    carry = np.zeros((B, d, d), dtype=dt)
    for t in range(T):
        L[:, t] = chol(D[:, t] - carry)
        if t < T - 1:
            G[:, t] = _T(solve_lower(L[:, t], _T(S[:, t])))
            carry = G[:, t] @ _T(G[:, t])
    lg = np.log(np.einsum("btii->bti", L))
    return L, G, np.sum(lg, axis=(-1, -2)), np.sum(np.abs(lg), axis=(-1, -2))


def forward(L, G, r):
    """y = L^{-1} r [B, T, d] and |y|^2 [B]."""
    T = L.shape[1]
    y = np.zeros_like(r)
    for t in range(T):
        rhs = r[:, t] if t == 0 else r[:, t] - np.einsum("bij,bj->bi", G[:, t - 1], y[:, t - 1])
        y[:, t] = solve_lower(L[:, t], rhs[..., None])[..., 0]
    return y, np.sum(y * y, axis=(-1, -2))


def selinv(L, G, y):
    """Diagonal blocks Sig_tt of (L L^T)^{-1} by the backward recursion, and x = L^{-T} y."""
    B, T, d = y.shape
    eye = np.broadcast_to(np.eye(d, dtype=L.dtype), (B, d, d))
    Sig, x = np.zeros_like(L), np.zeros_like(y)
    for t in range(T - 1, -1, -1):
        Li = solve_lower(L[:, t], eye)
        base = _T(Li) @ Li
        rhs = y[:, t]
        if t < T - 1:
            Gm = G[:, t] @ Li
            sub = -Sig[:, t + 1] @ Gm
            base = base - _T(sub) @ Gm
            rhs = rhs - np.einsum("bji,bj->bi", G[:, t], x[:, t + 1])
        Sig[:, t] = (base + _T(base)) / 2
        x[:, t] = solve_upper(L[:, t], rhs[..., None])[..., 0]
    return Sig, x


def project(H, x, Sig, dt=LD):
    """k_kf_project: Fmu = H x [B, T, o] and Fvar = diag(H Sig H^T) [B, T, o], each with the sum of its absolute terms."""
    H, x, Sig = np.asarray(H).astype(dt), np.asarray(x).astype(dt), np.asarray(Sig).astype(dt)
    Fmu = np.einsum("ai,bti->bta", H, x)
    aFmu = np.einsum("ai,bti->bta", np.abs(H), np.abs(x))
    Fvar = np.einsum("ai,aj,btij->bta", H, H, Sig)
    aFvar = np.einsum("ai,aj,btij->bta", np.abs(H), np.abs(H), np.abs(Sig))
    return SimpleNamespace(Fmu=Fmu, aFmu=aFmu, Fvar=Fvar, aFvar=aFvar)


def reference(cs, dt=LD):
    """Everything the four entry points give, in `dt`: m0 / m1 = assemble in modes 0 / 1; L, G; logdet, alogdet; quad (|y|^2 of the
    mode-0 right-hand side; its terms are squares, so it is its own sum of absolute terms); ll [B], all [B], total, atotal and the
    term counts n_ll, n_total; Sig, x, Fmu, Fvar of mode 1."""
    m0, m1 = assemble(cs, 0, dt), assemble(cs, 1, dt)
    L, G, logdet, alogdet = factor(m0.D, cs.Ps, dt)
    y0, quad = forward(L, G, m0.r)
    half = dt(0.5)
    slc = cs.sumlogchol.astype(dt)
    ll = dt(cs.cst) - half * m0.t1 + half * quad - slc - logdet + half * m0.ldR
    all_ = abs(dt(cs.cst)) + half * m0.at1 + half * quad + np.abs(slc) + alogdet + half * m0.aldR
    y1, _ = forward(L, G, m1.r)
    Sig, x = selinv(L, G, y1)
    pr = project(cs.H, x, Sig, dt)
    n_ll = 2 * cs.T * cs.o + 2 * cs.T * cs.d + 2
    return SimpleNamespace(m0=m0, m1=m1, L=L, G=G, logdet=logdet, alogdet=alogdet, quad=quad, y0=y0, ll=ll, all=all_, total=np.sum(ll),
                           atotal=np.sum(all_), n_ll=n_ll, n_total=cs.B * n_ll, Sig=Sig, x=x, Fmu=pr.Fmu, Fvar=pr.Fvar, aFmu=pr.aFmu,
                           aFvar=pr.aFvar)


# ---- the bounds (module docstring of tests/test_gpu_kf.py) -----------------------------------------------------------------------------
def ratio_local(got, want, absterms, n):
    """max |got - want| / (4 n EPS sum|terms|) over the entries; entries whose bound is 0 must be equal and count as 0."""
    got, want, absterms = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD), np.asarray(absterms, dtype=LD)
    assert got.shape == want.shape == absterms.shape, (got.shape, want.shape, absterms.shape)
    assert np.all(np.isfinite(got))
    bound = 4 * np.broadcast_to(np.asarray(n, dtype=LD), got.shape) * EPS * absterms
    err = np.abs(got - want)
    zero = bound == 0
    assert np.all(err[zero] == 0), "an entry with a zero bound differs"
    return float(np.max(np.where(zero, 0, err / np.where(zero, 1, bound))))


def ratio_array(got, want, cond):
    """Sweep bound of an array output [B, ...]: max|got - want| of a chain over 0.5 EPS cond_2 max|want| of that chain."""
    got, want = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    assert got.shape == want.shape and np.all(np.isfinite(got))
    B = got.shape[0]
    err = np.max(np.abs(got - want).reshape(B, -1), axis=1)
    scale = np.max(np.abs(want).reshape(B, -1), axis=1)
    return float(np.max(err / (0.5 * EPS * np.asarray(cond, dtype=LD) * scale)))


def ratio_scalar(got, want, absterms, n, cond):
    """Sweep bound of a per-chain scalar: |got - want| <= (0.5 cond_2 + 4 n) EPS sum|terms|."""
    got, want, absterms = np.atleast_1d(np.asarray(got, dtype=LD)), np.atleast_1d(np.asarray(want, dtype=LD)), np.atleast_1d(
        np.asarray(absterms, dtype=LD))
    assert got.shape == want.shape == absterms.shape and np.all(np.isfinite(got))
    return float(np.max(np.abs(got - want) / ((0.5 * np.asarray(cond, dtype=LD) + 4 * n) * EPS * absterms)))


def local_checks(cs, ref, D, r0, r1, t1, ldR):
    """{name: err / bound} of the outputs of k_kf_assemble (any of them may be None)."""
    o, out = cs.o, {}
    if D is not None:
        out["D"] = ratio_local(D, ref.m0.D, ref.m0.aD, o * o + 1)
    if r0 is not None:
        out["r mode 0"] = ratio_local(r0, ref.m0.r, ref.m0.ar, o * (o + 1) + 1)
    if r1 is not None:
        out["r mode 1"] = ratio_local(r1, ref.m1.r, ref.m1.ar, o * (o + 1) + 1)
    if t1 is not None:
        out["t1"] = ratio_local(t1, ref.m0.t1, ref.m0.at1, cs.T * o)
    if ldR is not None:
        out["ldR"] = ratio_local(ldR, ref.m0.ldR, ref.m0.aldR, cs.T * o)
    return out


def project_checks(cs, Fmu, Fvar, x, Sig):
    """{name: err / bound} of k_kf_project's outputs against the 80-bit projection of the x and Sig it read."""
    pr = project(cs.H, x, Sig)
    return {"Fmu of own x": ratio_local(Fmu, pr.Fmu, pr.aFmu, cs.d), "Fvar of own Sig": ratio_local(Fvar, pr.Fvar, pr.aFvar, cs.d * cs.d)}


def sweep_scalar_checks(cs, ref, logdet=None, quad=None, ll=None, total=None):
    nd, out = cs.T * cs.d, {}
    if logdet is not None:
        out["logdet"] = ratio_scalar(logdet, ref.logdet, ref.alogdet, nd, cs.cond)
    if quad is not None:
        out["quad"] = ratio_scalar(quad, ref.quad, ref.quad, nd, cs.cond)
    if ll is not None:
        out["ll"] = ratio_scalar(ll, ref.ll, ref.all, ref.n_ll, cs.cond)
    if total is not None:
        out["total"] = ratio_scalar(total, ref.total, ref.atotal, ref.n_total, cs.cond.max())
    return out


def sweep_array_checks(cs, ref, Sig=None, x=None, Fmu=None, Fvar=None):
    out = {}
    for name, got in (("Sig", Sig), ("x", x), ("Fmu", Fmu), ("Fvar", Fvar)):
        if got is not None:
            out[name] = ratio_array(got, getattr(ref, name), cs.cond)
    return out


# ---- the cases of tests/test_gpu_kf.py ---------------------------------------------------------------------------------------------------
# (B, T, R0, shared_sites, zero_mean)
CASES = (
    (3, 37, 4, True, False),      # ragged last segment (one node); shared sites, Hmu and plin given
    (3, 37, 4, False, True),      # the same partition; per-chain sites, Hmu and plin NULL
    (3, 37, 2, True, True),       # 19 segments: three levels; shared sites with Hmu and plin NULL
    (70, 9, 2, False, False),     # 350 lanes: b changes inside a 64-lane block, the last block is padded
    (2, 1, 0, False, False),      # T = 1, Ps NULL
    (2, 2, 0, False, False),      # single-level plan
    (2, 8, 8, False, False),      # T = R0: single-level plan, one full segment
)
LONG_CASE = (1, 16385, 2, False, False)       # P = 8193 >= 8192 with B == 1: the split sum; elbo's stage 1 at slice 129
LONG_DO = ((2, 1), (1, 2))
DIMS = tuple((d, o) for d in range(1, 9) for o in (1, 2))


def cases_of(d, o):
    return CASES + ((LONG_CASE,) if (d, o) in LONG_DO else ())
