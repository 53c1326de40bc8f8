"""
80-bit host reference of the VDP kernels (csrc/mfgm_vdp.h, the mfgm_packed_vdp_* entry points of include/mfgm.h) and the generator of
the inputs the host and GPU tests share.

Plain NumPy, sequential loops over t on [B, d, d] arrays, restating oracle/np_models.VariationalMarkovGP and the header comments of
include/mfgm.h with PER-DIMENSION drift parameters f_i(x) = af_i x - bf_i x^3 and diffusion q_i.  Every function takes the float type
`ft`: np.longdouble (the reference) or np.float64 (the fp64 twin: the same code, the yardstick of the tolerance rule of
tests/test_gpu_vdp.py).  Arrays are in natural node order: A [B, T-1, d, d] and b [B, T-1, d] of the transitions t -> t+1, marginals m
[B, T, d] and S [B, T, d, d], multipliers psi [B, T-1, d, d] and lam [B, T-1, d], jump terms yR [B, T, d] and dobsS [B, T, d, d].
`prm` is a SimpleNamespace(af, bf, q [d], mu0 [d], chol0 [d, d], dt, clip).
"""
from types import SimpleNamespace

import numpy as np

from tests.np_cq import LD, EPS, chol, tril_pack, rel_err, plan_levels, pack_nodes, unpack_nodes, SHAPES as CQ_SHAPES, forced_nodes  # noqa: F401
from tests.np_cq import spd_inverse

# np_cq.SHAPES plus a chain of one transition, where psi_0 and lam_0 are the terminal values and nothing else
SHAPES = list(CQ_SHAPES) + [(5, 2, 2, 0)]
SHAPE_IDS = ["B%d-T%d" % s[:2] for s in SHAPES]
N_RANDOM = 12
CLIP_CANDIDATES = (2.0, 3.0, 5.0, 1.5, 1.0, 0.75, 0.5, 0.35, 0.25, 0.15)
LRS = (0.3, 1.0)


def _T(x):
    return np.swapaxes(x, -1, -2)


def _diag(M):
    return np.einsum("...ii->...i", M)


def stab(x, c):
    """stabilize_system: NaN -> 1e-8, then clipping to [-c, c]."""
    return np.clip(np.where(np.isnan(x), x.dtype.type(1e-8), x), -c, c)


def _cast(prm, ft, *arrays):
    p = SimpleNamespace(af=np.asarray(prm.af, dtype=ft), bf=np.asarray(prm.bf, dtype=ft), q=np.asarray(prm.q, dtype=ft),
                        mu0=np.asarray(prm.mu0, dtype=ft), chol0=np.asarray(prm.chol0, dtype=ft), dt=ft(prm.dt), clip=ft(prm.clip))
    return (p,) + tuple(np.asarray(a, dtype=ft) for a in arrays)


def transitions(A, b, prm, ft=LD):
    """T_t = I - dt A_t [B, T-1, d, d] and o_{t+1} = dt b_t [B, T-1, d]; with clip > 0 NaN -> 1e-8 and clipped to [-1, 1]."""
    p, A, b = _cast(prm, ft, A, b)
    Tm = -p.dt * A
    d = A.shape[-1]
    Tm[..., np.arange(d), np.arange(d)] += ft(1)
    o = p.dt * b
    if p.clip > 0:
        Tm, o = stab(Tm, ft(1)), stab(o, ft(1))
    return Tm, o


def to_ssm(A, b, prm, ft=LD):
    """mfgm_packed_vdp_to_ssm: (A [B, T, d, d] with a zero last node, off [B, T, d] with mu0 at node 0, chol [B, T, d, d] lower with
    chol0 at node 0 and diag sqrt(dt q_i) elsewhere)."""
    p, A, b = _cast(prm, ft, A, b)
    Tm, o = transitions(A, b, prm, ft)
    B, N, d = b.shape
    At = np.concatenate([Tm, np.zeros((B, 1, d, d), dtype=ft)], axis=1)
    off = np.concatenate([np.broadcast_to(p.mu0, (B, 1, d)), o], axis=1)
    ch = np.zeros((B, N + 1, d, d), dtype=ft)
    ch[:, 0] = p.chol0
    ch[:, 1:] = np.sqrt(p.dt * p.q)[:, None] * np.eye(d, dtype=ft)
    return At, off, ch


def to_naturals(A, b, prm, P0inv, P0lin, ft=LD):
    """mfgm_packed_vdp_to_naturals (csrc/mfgm_vdp.h:173-177): with W = diag(1 / (dt q)),
    diag_t = [t = 0 ? P0^-1 : W] + T_t^T W T_t [t < T-1], sub_t = -W T_t (zero at T-1), lin_t = [t = 0 ? P0^-1 mu0 : W o_t] - T_t^T W o_{t+1}."""
    p, A, b, P0inv, P0lin = _cast(prm, ft, A, b, P0inv, P0lin)
    Tm, o = transitions(A, b, prm, ft)
    B, N, d = b.shape
    W = ft(1) / (p.dt * p.q)
    diag = np.zeros((B, N + 1, d, d), dtype=ft)
    lin = np.zeros((B, N + 1, d), dtype=ft)
    sub = np.zeros((B, N + 1, d, d), dtype=ft)
    diag[:, 0], lin[:, 0] = P0inv, P0lin
    diag[:, 1:] = W[:, None] * np.eye(d, dtype=ft)
    lin[:, 1:] = W * o
    WT = W[:, None] * Tm
    sub[:, :N] = -WT
    diag[:, :N] += _T(Tm) @ WT
    lin[:, :N] -= (_T(WT) @ o[..., None])[..., 0]
    return lin, diag, sub


def drift_moments(m, v, prm):
    """Gaussian moments of the per-dimension cubic under N(m_i, v_i): E f, E f', Var f and the partial derivatives the gradients need."""
    al, be = prm.af, prm.bf
    m2 = m * m
    a = m2 + v
    return SimpleNamespace(
        Ef=al * m - be * m * (m2 + 3 * v), Jf=al - 3 * be * a,
        Vf=al * al * v - 6 * al * be * v * a + be * be * v * (9 * m2 * m2 + 36 * m2 * v + 15 * v * v),
        Ef_v=-3 * be * m, J_m=-6 * be * m, J_v=-3 * be + 0 * m,
        V_m=-12 * al * be * m * v + be * be * m * v * (36 * m2 + 72 * v),
        V_v=al * al - 6 * al * be * (m2 + 2 * v) + be * be * (9 * m2 * m2 + 72 * m2 * v + 45 * v * v))


def energy_terms(m, S, A, b, prm, ft=LD, grads=True):
    """Per node e_t = 1/2 sum_i (1 / q_i) E (f_L,i - f_i)^2 with f_L = -A x + b, m [..., d], S [..., d, d]; and de/dm, de/dS
    (symmetric convention), restating oracle/np_sde.e_sde_closed_form with per-dimension af, bf."""
    p, m, S, A, b = _cast(prm, ft, m, S, A, b)
    d = m.shape[-1]
    w = ft(1) / p.q
    mo = drift_moments(m, _diag(S), p)
    l = -A
    El = (l @ m[..., None])[..., 0] + b
    LS = l @ S
    LSL = np.sum(LS * l, axis=-1)
    LSii = _diag(LS)
    r = El - mo.Ef
    e = np.sum(w * (LSL - 2 * LSii * mo.Jf + mo.Vf + r * r), axis=-1) / 2
    if not grads:
        return e, None, None
    dm = ((w * r)[..., None, :] @ l)[..., 0, :]
    dm = dm + w * (-2 * r * mo.Jf - 2 * LSii * mo.J_m + mo.V_m) / 2
    wl = w[:, None] * l
    wJl = (w * mo.Jf)[..., :, None] * l                  # row i: w_i Jf_i l_i
    dS = (_T(l) @ wl - wJl - _T(wJl)) / 2
    dS[..., np.arange(d), np.arange(d)] += w * (-2 * LSii * mo.J_v + mo.V_v - 2 * r * mo.Ef_v) / 2
    return e, dm, dS


def esde(m, S, A, b, prm, ft=LD):
    """mfgm_packed_vdp_esde: (e_over_dt [B], dE/dm / dt [B, T-1, d], dE/dS / dt [B, T-1, d, d]) over the nodes 0 ... T-2."""
    N = np.shape(b)[1]
    m, S = np.asarray(m)[:, :N], np.asarray(S)[:, :N]
    e, dm, dS = energy_terms(m, S, A, b, prm, ft)
    return e.sum(axis=1), dm, dS


def marginals(A, b, prm, q0_mu, q0_cov, ft=LD):
    """mfgm_packed_vdp_marginals: m_{t+1} = T_t m_t + o_{t+1}, S_{t+1} = T_t S_t T_t^T + diag(dt q); e_over_dt of these marginals."""
    p, A, b, q0_mu, q0_cov = _cast(prm, ft, A, b, q0_mu, q0_cov)
    Tm, o = transitions(A, b, prm, ft)
    B, N, d = b.shape
    m = np.empty((B, N + 1, d), dtype=ft)
    S = np.empty((B, N + 1, d, d), dtype=ft)
    m[:, 0], S[:, 0] = q0_mu, q0_cov
    Q = (p.dt * p.q)[:, None] * np.eye(d, dtype=ft)
    for t in range(N):
        m[:, t + 1] = (Tm[:, t] @ m[:, t, :, None])[..., 0] + o[:, t]
        S[:, t + 1] = Tm[:, t] @ S[:, t] @ _T(Tm[:, t]) + Q
    e = energy_terms(m[:, :N], S[:, :N], A, b, prm, ft, grads=False)[0].sum(axis=1)
    return m, S, e


def lagrange(m, S, A, b, prm, yR, dobsS, ft=LD):
    """mfgm_packed_vdp_lagrange, the loop of np_models.VariationalMarkovGP.update_lagrange: psi_{N-1} = 1e-10 I, lam_{N-1} = 0,
    d_obs_m = yR + 2 dobsS m, d_obs_S = dobsS, every one of dE/dm, dE/dS, d_obs_m, d_obs_S clipped on its own when clip > 0.  Returns
    SimpleNamespace(psi, lam, pre = the four quantities before clipping at the nodes 1 ... N-1 the loop reads)."""
    p, m, S, A, b, yR, dobsS = _cast(prm, ft, m, S, A, b, yR, dobsS)
    B, N, d = b.shape
    _, dEdm, dEdS = esde(m, S, A, b, prm, ft)
    d_obs_m = yR + 2 * (dobsS @ m[..., None])[..., 0]
    d_obs_S = dobsS
    pre = dict(dEdm=dEdm[:, 1:], dEdS=dEdS[:, 1:], d_obs_m=d_obs_m[:, 1:N], d_obs_S=d_obs_S[:, 1:N])
    if p.clip > 0:
        dEdm, dEdS, d_obs_m, d_obs_S = (stab(x, p.clip) for x in (dEdm, dEdS, d_obs_m, d_obs_S))
    psi = np.empty((B, N, d, d), dtype=ft)
    lam = np.zeros((B, N, d), dtype=ft)
    psi[:] = ft(1e-10) * np.eye(d, dtype=ft)
    for t in range(N - 1, 0, -1):
        pa = psi[:, t] @ A[:, t]
        d_psi = pa + pa - dEdS[:, t]
        d_lam = (A[:, t] @ lam[:, t, :, None])[..., 0] - dEdm[:, t]
        psi[:, t - 1] = psi[:, t] - p.dt * d_psi - d_obs_S[:, t]
        lam[:, t - 1] = lam[:, t] - p.dt * d_lam - d_obs_m[:, t]
    return SimpleNamespace(psi=psi, lam=lam, pre=pre)


def update_param(m, S, psi, lam, A, b, prm, lr, ft=LD):
    """mfgm_packed_vdp_update_param: (A', b', psi, lam) with psi / lam clipped first when clip > 0; A~ = 2 diag(q) psi - diag(E f'),
    b~ = E f + A~ m - q o lam, blended with lr."""
    p, m, S, psi, lam, A, b = _cast(prm, ft, m, S, psi, lam, A, b)
    N, d = b.shape[1], b.shape[2]
    m, S = m[:, :N], S[:, :N]
    if p.clip > 0:
        psi, lam = stab(psi, p.clip), stab(lam, p.clip)
    mo = drift_moments(m, _diag(S), p)
    At = 2 * p.q[:, None] * psi
    At[..., np.arange(d), np.arange(d)] -= mo.Jf
    bt = mo.Ef + (At @ m[..., None])[..., 0] - p.q * lam
    lr = ft(lr)
    return (1 - lr) * A + lr * At, (1 - lr) * b + lr * bt, psi, lam


# ---- the generator ------------------------------------------------------------------------------------------------------------------------
def observation_nodes(T, level0):
    """(forced nodes, the forced node that carries two observations).  A chain of one transition has nodes 0 and 1 only."""
    if T == 2:
        return np.array([0, 1]), 1
    forced = np.union1d(forced_nodes(T, level0), [T - 2])     # (the last node the Lagrange loop reads)
    _, R, P, _ = level0
    p = P // 2 if P > 2 else 0
    return forced, p * R + R - 1                             # the last node of an interior segment


def _build(d, shape, variant, seed, kind):
    B, T, R0, Rup = shape
    levels = plan_levels(B, T, d, R0, Rup)
    N, dt = T - 1, 0.05
    rng = np.random.default_rng([40713, d, B, T, seed, kind == "ou"])
    af, bf, q = 0.5 + rng.random(d), 0.3 + 0.7 * rng.random(d), 0.4 + 0.8 * rng.random(d)
    if kind == "ou":
        af, bf = -af, np.zeros(d)
    L0 = np.tril(rng.normal(size=(d, d)), -1) * 0.1 + np.diag(0.6 + 0.4 * rng.random(d))
    prm = SimpleNamespace(af=af, bf=bf, q=q, mu0=0.3 * rng.normal(size=d), chol0=L0, dt=dt, clip=0.0)
    A = 0.6 * rng.normal(size=(B, N, d, d)) / np.sqrt(d)
    A[..., np.arange(d), np.arange(d)] = 2.0 + 2.0 * rng.random((B, N, d))
    b = rng.normal(size=(B, N, d))
    if variant == "stab":
        A = np.triu(3.0 * rng.normal(size=(B, N, d, d)), 1)
        A[..., np.arange(d), np.arange(d)] = 4.0 + 2.0 * rng.random((B, N, d))
        A = np.where(np.triu(rng.random(A.shape) < 0.15, 1), 150.0 * np.sign(rng.normal(size=A.shape)), A)
        A = np.where(np.triu(rng.random(A.shape) < 0.02, 1), np.nan, A)
        b = np.where(rng.random(b.shape) < 0.02, np.nan, 25.0 * b)
        prm.clip = 5000.0
    q0_mu = 0.5 * rng.normal(size=(B, d))
    Lq = np.tril(rng.normal(size=(B, d, d)), -1) * 0.1 + (0.5 + 0.5 * rng.random((B, d)))[:, :, None] * np.eye(d)
    q0_cov = Lq @ _T(Lq)
    p0inv = spd_inverse(q0_cov).astype(np.float64)
    p0lin = (p0inv @ q0_mu[..., None])[..., 0]
    # jump terms
    M = rng.normal(size=(d, d))
    Rinv = M @ M.T / d + 0.5 * np.eye(d)
    forced, twice = observation_nodes(T, levels[0])
    free = np.setdiff1d(np.arange(T), forced)
    k = min(N_RANDOM, (len(free) + 1) // 2)
    obs_count = np.zeros((B, T), dtype=np.int32)
    yR = np.zeros((B, T, d))
    obs_t = []
    for c in range(B):
        rnd = rng.choice(free, size=k, replace=False) if k else np.zeros(0, dtype=int)
        nodes = np.concatenate([forced, [twice], rnd, rnd[:1]])
        obs_t.append(nodes)
        y = np.sign(rng.normal(size=(len(nodes), d))) + 0.1 * rng.normal(size=(len(nodes), d))
        np.add.at(obs_count[c], nodes, 1)
        np.add.at(yR[c], nodes, y @ Rinv)
    if variant == "noobs":
        obs_count[:], yR[:] = 0, 0.0
    dobs_const = -0.5 * Rinv
    dobsS = obs_count[..., None, None] * dobs_const
    case = SimpleNamespace(d=d, B=B, T=T, shape=shape, variant=variant, kind=kind, levels=levels, prm=prm, A=A, b=b, q0_mu=q0_mu,
                           q0_cov=q0_cov, p0inv=p0inv, p0lin=p0lin, Rinv=Rinv, obs_t=np.stack(obs_t), obs_count=obs_count, yR=yR,
                           dobs_const=dobs_const, dobsS=dobsS, forced=forced, twice=twice)
    case.prm_m = prm
    return case


CLIP_SEEDS = 40


def make_case(d, shape, variant, seed=0, kind="dw"):
    """Everything a GPU call needs, nothing negligibly small and nothing shared between dimensions: dt = 0.05, af in [0.5, 1.5], bf in
    [0.3, 1.0], q in [0.4, 1.2], all distinct (kind "ou": af in [-1.5, -0.5], bf = 0); A_t = diag in [2, 4] + 0.6 randn / sqrt(d) (not
    symmetric), b_t ~ randn; q0_mu [B, d] and a dense SPD q0_cov per chain; R^-1 = M M^T / d + I / 2 dense, yR = R^-1 y with
    y ~ +-1 + 0.1 randn; observations at np_cq.forced_nodes plus N_RANDOM random nodes per chain, one forced node and one random node
    carrying two (so obs_count = 2 occurs, and at d = 1, where d_obs_S takes one value per count, it is a share of the observed nodes
    that a clip value can separate).
    variant "full" | "noobs" (no observation on any chain) | "clip" (small clip values, picked from CLIP_CANDIDATES, that meet
    clip_conditions; see below) | "stab" (forward kernels: A upper triangular with 15 % of the strictly upper entries at +-150, 2 % NaN
    in A's strictly upper entries and in b, offsets dt b beyond +-1 at part of the nodes, clip = 5000).
    "clip" carries two values, because no single one can meet the conditions on all six clipped quantities: between observations the
    sweep settles at psi ~ dE/dS / (2 A) with A in [2, 4], so a value below which 5 % of psi are clipped clips every dE/dS at d = 1
    (measured on the T = 257 shape: dE/dS 100 % clipped at every value that clips any psi).  case.prm.clip meets the conditions on
    dE/dm, dE/dS, d_obs_m, d_obs_S (the Lagrange sweep and the fused routes run with it), case.prm_m.clip those on psi and lam (the
    stand-alone mfgm_packed_vdp_update_param runs with it, on the multipliers the sweep with prm.clip gave).  Whether the first pair can
    be met at all depends on the draw of R^-1 (at d = 1 d_obs_S takes two values): the generator walks the seeds seed, seed + 1, ...
    (at most CLIP_SEEDS) and the candidates in order and takes the first that meets every condition; it fails if there is none.
    The case carries its 80-bit reference (case.ref, see reference()) and has been through check_case."""
    if variant != "clip" or shape[1] == 2:
        case = _build(d, shape, variant, seed, kind)
        if variant == "clip":                                    # (the Lagrange loop of a chain of one transition reads nothing)
            case.prm.clip = 2.0
            case.prm_m = SimpleNamespace(**vars(case.prm))
        case.ref = reference(case)
        check_case(case, case.ref)
        return case
    why = []
    for s in range(seed, seed + CLIP_SEEDS):
        case = _build(d, shape, variant, s, kind)
        c, p = case, case.prm
        m, S, _ = marginals(c.A, c.b, p, c.q0_mu, c.q0_cov)
        m64, S64 = m.astype(np.float64), S.astype(np.float64)
        for clip in CLIP_CANDIDATES:
            p.clip = clip
            lg = lagrange(m64, S64, c.A, c.b, p, c.yR, c.dobsS)
            bad = clip_conditions(case, lg.pre, None, None, clip)
            if bad:
                why.append((s, clip, bad))
                continue
            for clip_m in CLIP_CANDIDATES:
                bad = clip_conditions(case, None, lg.psi, lg.lam, clip_m)
                if not bad:
                    case.prm_m = SimpleNamespace(**vars(p))
                    case.prm_m.clip = clip_m
                    case.seed = s
                    case.ref = reference(case)
                    check_case(case, case.ref)
                    return case
                why.append((s, clip, clip_m, bad))
    raise AssertionError(("no seed and clip values meet the conditions", d, shape, why[-3:]))


def reference(case, ft=LD):
    """Every reference output of a case in float type ft.  The stages after the forward pass take the 80-bit marginals (and multipliers)
    ROUNDED TO fp64 as their inputs, as the GPU calls do: r.m64, r.S64, r.psi64, r.lam64 (the same arrays whatever ft)."""
    c, p = case, case.prm
    r = SimpleNamespace()
    r.ssm = to_ssm(c.A, c.b, p, ft)
    r.nat = to_naturals(c.A, c.b, p, c.p0inv, c.p0lin, ft)
    r.m, r.S, r.e_fwd = marginals(c.A, c.b, p, c.q0_mu, c.q0_cov, ft)
    if c.variant == "stab":
        return r
    if ft is LD:
        r.m64, r.S64 = r.m.astype(np.float64), r.S.astype(np.float64)
    else:
        r.m64, r.S64 = case.ref.m64, case.ref.S64
    r.e, r.gm, r.gS = esde(r.m64, r.S64, c.A, c.b, p, ft)
    lg = lagrange(r.m64, r.S64, c.A, c.b, p, c.yR, c.dobsS, ft)
    r.psi, r.lam, r.pre = lg.psi, lg.lam, lg.pre
    if ft is LD:
        r.psi64, r.lam64 = r.psi.astype(np.float64), r.lam.astype(np.float64)
    else:
        r.psi64, r.lam64 = case.ref.psi64, case.ref.lam64
    # update_param on the rounded multipliers (the stand-alone kernel) and on the sweep's own (the fused routes)
    r.upd = {lr: update_param(r.m64, r.S64, r.psi64, r.lam64, c.A, c.b, c.prm_m, lr, ft) for lr in LRS}
    r.fused = {lr: update_param(r.m64, r.S64, r.psi, r.lam, c.A, c.b, p, lr, ft) for lr in LRS}
    return r


def outputs(r):
    """name -> array of every reference output (the table the host test prints and the GPU tests look their yardsticks up in)."""
    out = {"ssm A": r.ssm[0], "ssm off": r.ssm[1], "ssm chol": r.ssm[2], "nat lin": r.nat[0], "nat diag": r.nat[1], "nat sub": r.nat[2],
           "m": r.m, "S": r.S, "e_fwd": r.e_fwd}
    if hasattr(r, "e"):
        out.update({"e": r.e, "gm": r.gm, "gS": r.gS, "psi": r.psi, "lam": r.lam})
        for tag, res in (("upd", r.upd), ("fused", r.fused)):
            for lr, (A2, b2, pc, lc) in res.items():
                out.update({f"{tag} lr={lr} A": A2, f"{tag} lr={lr} b": b2, f"{tag} lr={lr} psi": pc, f"{tag} lr={lr} lam": lc})
    return out


def clip_conditions(case, pre, psi, lam, clip):
    """The conditions of the "clip" variant as a list of violations (empty: they hold), for the quantities given (pre: the four the
    Lagrange sweep clips, before clipping; psi, lam: the multipliers update_param clips): between 5 % and 95 % of the entries of each
    are clipped in the reference, and no value before clipping lies within 1e-9 relative of +-clip.  The entries counted are those the
    sweep reads and that can be non-zero: dE/dm, dE/dS at the nodes 1 ... N-1, d_obs_m, d_obs_S at the observed ones among them (they
    are exactly zero elsewhere), psi and lam at the nodes 0 ... N-2 (node N-1 holds the terminal value)."""
    c = LD(clip)
    sets = {}
    if pre is not None:
        obs = case.obs_count[:, 1:case.T - 1] > 0
        sets.update({"dEdm": pre["dEdm"], "dEdS": pre["dEdS"], "d_obs_m": pre["d_obs_m"][obs], "d_obs_S": pre["d_obs_S"][obs]})
    if psi is not None:
        sets.update({"psi": psi[:, :-1], "lam": lam[:, :-1]})
    bad = []
    for name, x in sets.items():
        x = np.abs(np.asarray(x, dtype=LD)).reshape(-1)
        frac = float(np.mean(x > c)) if x.size else 0.0
        if not 0.05 <= frac <= 0.95:
            bad.append((name, "clipped share", round(frac, 4)))
        if x.size and np.abs(x - c).min() <= LD(1e-9) * c:
            bad.append((name, "within 1e-9 of the clip value"))
    return bad


def check_case(case, r):
    """The generator's assertions, on the 80-bit values: |I - 2 dt A_t|_2 < 1 and every eigenvalue of every S_t above 0.02 (outside
    "stab"); no reference output negligibly small: the inputs are of order one, so the typical entry of an output is, and max |output|
    must be at least 1e-3 (the multipliers of a chain of one transition are the terminal values 1e-10 I and 0: they are compared
    exactly, not relatively); the "clip" conditions."""
    d, T = case.d, case.T
    if case.variant != "stab":
        X = np.eye(d) - 2 * case.prm.dt * case.A
        assert np.linalg.norm(X, 2, axis=(-2, -1)).max() < 1.0, "I - 2 dt A_t is not a contraction"
        assert np.linalg.eigvalsh(r.S.astype(np.float64)).min() > 0.02, "an S_t is nearly singular"
    for name, x in outputs(r).items():
        x = np.asarray(x)
        if case.variant == "stab" and name == "e_fwd":
            continue                                             # the energy of a NaN drift is NaN
        assert np.all(np.isfinite(x.astype(np.float64))), name
        if T == 2 and (name.endswith("psi") or name.endswith("lam") or (case.kind == "ou" and name.endswith("lr=1.0 b"))):
            continue                                             # (and b~ = 2 q psi m - q lam of a linear drift vanishes with them)
        assert np.abs(x).max() >= 1e-3, (name, float(np.abs(x).max()))
    if case.variant == "clip" and T > 2:
        bad = clip_conditions(case, r.pre, None, None, case.prm.clip) + clip_conditions(case, None, r.psi64, r.lam64, case.prm_m.clip)
        assert not bad, bad
    if T > 2 and case.variant in ("full", "clip"):
        # the observation edges: nodes 0, 1, 2, T-2, T-1 observed on every chain, adjacent nodes, a node with two observations
        assert np.all(case.obs_count[:, [0, 1, 2, T - 2, T - 1]] >= 1) and np.all(case.obs_count[:, case.twice] >= 2)
    return True


def yardsticks(case):
    """name -> rel_err of the fp64 twin against the 80-bit reference, for every output of outputs() with a non-zero reference (the
    multipliers of a chain of one transition, and the energy of the NaN drifts of "stab", are left out)."""
    want, twin = outputs(case.ref), outputs(reference(case, np.float64))
    out = {}
    for name, w in want.items():
        if not np.all(np.isfinite(np.asarray(w, dtype=np.float64))) or np.abs(w).max() == 0:
            continue
        out[name] = rel_err(twin[name], w)
    return out
