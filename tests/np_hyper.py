"""
NumPy helpers of the hyper-parameter score tests (tests/test_host_hyper.py, tests/test_gpu_hyper.py); not a test module.

A kernel tree is a nested tuple:
    ("M12" | "M32" | "M52", lengthscale, variance)   ("OU", decay, diffusion)   ("H", variance, period)   ("C", variance)
    ("Sum", [children])   ("Prod", [children])
with the hyper-parameters in the order of vidp_amd's hyperparameter_leaves().

  (i)   dense_ll_and_grad   log marginal likelihood and its gradient from the dense covariance K + sigma^2 I:
                            1/2 tr((alpha alpha^T - K_y^-1) dK) with dK by the complex step (exact to rounding, the product rule comes
                            with the complex arithmetic); no finite differences of ll.  K in closed form for a jitter-free tree, from
                            the state-space recursion (which the jitter enters) otherwise.
  (ii)  score_restatement   the formulas of csrc/mfgm_score.h on given centred pairwise moments (x, Sig, Sub), in fp64 ...
  (iii)                     ... or in np.longdouble (dtype=np.longdouble; its own Cholesky and substitutions, NumPy's LAPACK has none).
"""
import numpy as np

from oracle import np_kalman, np_kernels
from tests import np_kernels_ext as E

LEAF_DIM = {"M12": 1, "OU": 1, "M32": 2, "M52": 3, "H": 2, "C": 1}
EXACT = ("H", "C")


# -- trees ------------------------------------------------------------------------------------------------------------------------------
def is_leaf(spec):
    return spec[0] in LEAF_DIM


def flat_params(spec):
    """The hyper-parameters of the tree, depth first (the order of vidp_amd.hyper.flatten(kernel.hyperparameter_leaves()))."""
    if is_leaf(spec):
        return list(spec[1:])
    out = []
    for c in spec[1]:
        out.extend(flat_params(c))
    return out


def with_params(spec, params):
    """The same tree with its hyper-parameters replaced from the flat list `params` (consumed from the front; any scalar type)."""
    if is_leaf(spec):
        n = len(spec) - 1
        vals = [params.pop(0) for _ in range(n)]
        return (spec[0],) + tuple(vals)
    return (spec[0], [with_params(c, params) for c in spec[1]])


def terms_of(spec):
    """[[leaf, ...] per term]: a Sum's terms, each the factors of a Product (the order of vidp_amd's _terms())."""
    if is_leaf(spec):
        return [[spec]]
    if spec[0] == "Sum":
        out = []
        for c in spec[1]:
            out.extend(terms_of(c))
        return out
    factors = []
    for c in spec[1]:
        t = terms_of(c)
        assert len(t) == 1
        factors.extend(t[0])
    return [factors]


def state_dim(spec):
    return sum(int(np.prod([LEAF_DIM[f[0]] for f in term])) for term in terms_of(spec))


def shortest_lengthscale(spec):
    """The shortest time scale of the tree (lengthscale, 1 / decay or period)."""
    if is_leaf(spec):
        return {"M12": lambda s: s[1], "M32": lambda s: s[1], "M52": lambda s: s[1], "OU": lambda s: 1.0 / s[1],
                "H": lambda s: s[2], "C": lambda s: np.inf}[spec[0]](spec)
    return min(shortest_lengthscale(c) for c in spec[1])


def build_np(spec, jitter=0.0):
    """The oracle's kernel (oracle.np_kernels / tests.np_kernels_ext)."""
    k = spec[0]
    if k in ("M12", "M32", "M52"):
        return {"M12": np_kernels.Matern12, "M32": np_kernels.Matern32, "M52": np_kernels.Matern52}[k](spec[1], spec[2], jitter=jitter)
    if k == "OU":
        return np_kernels.OrnsteinUhlenbeck(spec[1], spec[2], jitter=jitter)
    if k == "H":
        return E.HarmonicOscillator(spec[1], spec[2], jitter=jitter)
    if k == "C":
        return E.Constant(spec[1], jitter=jitter)
    kids = [build_np(c) for c in spec[1]]
    return np_kernels.Sum(kids, jitter=jitter) if k == "Sum" else E.Product(kids, jitter=jitter)


def build_vidp(spec, jitter=0.0):
    """The package's kernel."""
    from vidp_amd import kernels as K
    k = spec[0]
    if k in ("M12", "M32", "M52"):
        return {"M12": K.Matern12, "M32": K.Matern32, "M52": K.Matern52}[k](spec[1], spec[2], jitter=jitter)
    if k == "OU":
        return K.OrnsteinUhlenbeck(spec[1], spec[2], jitter=jitter)
    if k == "H":
        return K.HarmonicOscillator(spec[1], spec[2], jitter=jitter)
    if k == "C":
        return K.Constant(spec[1], jitter=jitter)
    kids = [build_vidp(c) for c in spec[1]]
    return K.Sum(kids, jitter=jitter) if k == "Sum" else K.Product(kids, jitter=jitter)


# -- factor blocks: the closed forms of factor_blocks / factor_der (csrc/mfgm_kernel_ssm.h, csrc/mfgm_score.h), any scalar type -----------
def rate_var(leaf):
    """(rate, var) of a leaf as the device sees it (include/mfgm.h)."""
    k = leaf[0]
    if k == "M12":
        return 1.0 / leaf[1], leaf[2]
    if k == "M32":
        return np.sqrt(3.0) / leaf[1], leaf[2]
    if k == "M52":
        return np.sqrt(5.0) / leaf[1], leaf[2]
    if k == "OU":
        return leaf[1], leaf[2] / (2.0 * leaf[1])
    if k == "H":
        return 2.0 * np.pi / leaf[2], leaf[1]
    return 0.0 * leaf[1], leaf[1]


def leaf_grads(leaf, g_rate, g_var):
    """The chain rule from (rate, var) to the leaf's own hyper-parameters, in their order."""
    k = leaf[0]
    rate, _ = rate_var(leaf)
    if k in ("M12", "M32", "M52"):
        return [-g_rate * rate / leaf[1], g_var]
    if k == "OU":
        return [g_rate - g_var * leaf[2] / (2.0 * leaf[1] ** 2), g_var / (2.0 * leaf[1])]
    if k == "H":
        return [g_var, -g_rate * rate / leaf[2]]
    return [g_var]


def factor_blocks(kind, l, v, dt, dtype):
    """(a, p) of one factor: row-major DF x DF arrays of `dtype` (complex allowed)."""
    n = LEAF_DIM[kind]
    a, p = np.zeros((n, n), dtype=dtype), np.zeros((n, n), dtype=dtype)
    if kind in ("M12", "OU"):
        a[0, 0], p[0, 0] = np.exp(-l * dt), v
    elif kind == "C":
        a[0, 0], p[0, 0] = 1.0, v
    elif kind == "M32":
        ex = np.exp(-l * dt)
        a[:] = [[ex * (1 + l * dt), ex * dt], [ex * (-l * l * dt), ex * (1 - l * dt)]]
        p[0, 0], p[1, 1] = v, v * l * l
    elif kind == "H":
        s, c = np.sin(l * dt), np.cos(l * dt)
        a[:] = [[c, -s], [s, c]]
        p[0, 0], p[1, 1] = v, v
    else:
        ex = np.exp(-l * dt)
        l2, l3, l4, h = l * l, l * l * l, l * l * l * l, 0.5 * dt * dt
        a[:] = [[ex * (1 + l * dt + l2 * h), ex * (dt + 2 * l * h), ex * h],
                [ex * (-l3 * h), ex * (1 + l * dt - 2 * l2 * h), ex * (dt - l * h)],
                [ex * (-l3 * dt + l4 * h), ex * (-3 * l2 * dt + 2 * l3 * h), ex * (1 - 2 * l * dt + l2 * h)]]
        l23 = l * l / 3
        p[0, 0], p[0, 2], p[2, 0], p[1, 1], p[2, 2] = v, -v * l23, -v * l23, v * l23, v * l4
    return a, p


def factor_der(kind, l, v, dt, dtype):
    """(da / d rate, dp / d rate, dp / d var), the simplified closed forms of factor_der."""
    n = LEAF_DIM[kind]
    da, dpl, dpv = (np.zeros((n, n), dtype=dtype) for _ in range(3))
    if kind in ("M12", "OU"):
        da[0, 0], dpv[0, 0] = -dt * np.exp(-l * dt), 1.0
    elif kind == "C":
        dpv[0, 0] = 1.0
    elif kind == "M32":
        ex, u = np.exp(-l * dt), l * dt
        da[:] = [[ex * (-u * dt), ex * (-dt * dt)], [ex * (u * (u - 2)), ex * (dt * (u - 2))]]
        dpl[1, 1] = 2 * v * l
        dpv[0, 0], dpv[1, 1] = 1.0, l * l
    elif kind == "H":
        s, c = np.sin(l * dt), np.cos(l * dt)
        da[:] = [[-dt * s, -dt * c], [dt * c, -dt * s]]
        dpv[0, 0], dpv[1, 1] = 1.0, 1.0
    else:
        ex, u, h, l2 = np.exp(-l * dt), l * dt, 0.5 * dt * dt, l * l
        q = -3 + 3 * u - 0.5 * u * u
        da[:] = [[ex * (-l2 * dt * h), ex * (-2 * u * h), ex * (-dt * h)],
                 [ex * (l2 * h * (u - 3)), ex * (2 * l * h * (u - 3)), ex * (h * (u - 3))],
                 [ex * (l2 * dt * q), ex * (u * (-6 + 6 * u - u * u)), ex * (dt * q)]]
        t = 2 * v * l / 3
        dpl[0, 2], dpl[2, 0], dpl[1, 1], dpl[2, 2] = -t, -t, t, 4 * v * l2 * l
        dpv[0, 0], dpv[0, 2], dpv[2, 0], dpv[1, 1], dpv[2, 2] = 1.0, -l2 / 3, -l2 / 3, l2 / 3, l2 * l2
    return da, dpl, dpv


def kron_all(mats):
    out = mats[0]
    for m in mats[1:]:
        out = np.kron(out, m)
    return out


def term_blocks(term, dt, dtype):
    """(A, P, Qterm, [a_f], [p_f]) of one term under the exact-Q rule (include/mfgm.h, mfgm_packed_kernel_ssm): Q without jitter."""
    blocks = []
    for leaf in term:
        r, v = rate_var(leaf)
        blocks.append(factor_blocks(leaf[0], dtype(r), dtype(v), dt, dtype))
    a, p = [b[0] for b in blocks], [b[1] for b in blocks]
    A, P = kron_all(a), kron_all(p)
    inexact = [i for i, leaf in enumerate(term) if leaf[0] not in EXACT]
    if not inexact:
        Q = np.zeros_like(P)
    elif len(inexact) == 1:
        g = inexact[0]
        Q = kron_all([p[i] - a[i] @ p[i] @ a[i].T if i == g else p[i] for i in range(len(term))])
    else:
        Q = P - kron_all([p[i] if term[i][0] in EXACT else a[i] @ p[i] @ a[i].T for i in range(len(term))])
    return A, P, Q, a, p


# -- (ii) / (iii): the device formulas on given moments --------------------------------------------------------------------------------------
def _cholesky(K):
    n = K.shape[0]
    L = np.zeros_like(K)
    for j in range(n):
        s = K[j, j] - (L[j, :j] * L[j, :j]).sum()
        assert s > 0
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, n):
            L[i, j] = (K[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return L


def _solve_lower(L, B):
    X = np.array(B, dtype=L.dtype, copy=True)
    for i in range(L.shape[0]):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def _solve_upper(U, B):
    X = np.array(B, dtype=U.dtype, copy=True)
    for i in range(U.shape[0] - 1, -1, -1):
        X[i] = (X[i] - U[i, i + 1:] @ X[i + 1:]) / U[i, i]
    return X


def _cotangent(L, M):
    """1/2 (K^-1 M K^-1 - K^-1), K = L L^T, through the whitened L^-1 M L^-T - I as the kernel forms it."""
    X = _solve_lower(L, _solve_lower(L, M).T).T
    X = X - np.eye(L.shape[0], dtype=L.dtype)
    return 0.5 * _solve_upper(L.T, _solve_upper(L.T, X).T).T


def score_restatement(spec, jitter, dts, x, Sig, Sub, dtype=np.float64):
    """The score of ONE chain with respect to every factor's (rate, var): array [nterm, 3, 2] in the order of terms_of(spec) (absent
    slots zero), from the centred moments x [T, d], Sig [T, d, d], Sub [T-1, d, d] = Sigma_{t+1,t} and the gaps dts [T-1]."""
    terms = terms_of(spec)
    T = x.shape[0]
    x, Sig = np.asarray(x, dtype=dtype), np.asarray(Sig, dtype=dtype)
    Sub = None if Sub is None else np.asarray(Sub, dtype=dtype)
    out = np.zeros((len(terms), 3, 2), dtype=dtype)
    jit = dtype(jitter)
    o = 0
    for c, term in enumerate(terms):
        n = int(np.prod([LEAF_DIM[f[0]] for f in term]))
        sl = slice(o, o + n)
        o += n
        eye = np.eye(n, dtype=dtype)

        def contract(Ga, Gp, a, p, dt):
            for f, leaf in enumerate(term):
                r, v = rate_var(leaf)
                da, dpl, dpv = factor_der(leaf[0], dtype(r), dtype(v), dt, dtype)
                rep = lambda blocks, new: kron_all([new if i == f else blocks[i] for i in range(len(term))])
                g = (Gp * rep(p, dpl)).sum()
                if Ga is not None:
                    g = g + (Ga * rep(a, da)).sum()
                out[c, f, 0] += g
                out[c, f, 1] += (Gp * rep(p, dpv)).sum()

        for t in range(T):
            mu = x[t, sl]
            Sc = Sig[t, sl, sl] + np.outer(mu, mu)
            if t == 0:
                _, P, _, a, p = term_blocks(term, dtype(0.0), dtype)
                contract(None, _cotangent(_cholesky(P + jit * eye), Sc), a, p, dtype(0.0))
                continue
            dt = dtype(dts[t - 1])
            A, P, Q, a, p = term_blocks(term, dt, dtype)
            Q = Q + jit * eye
            if not Q.any():
                continue                      # exact-Q rule: a zero block carries no score
            mup = x[t - 1, sl]
            Sp = Sig[t - 1, sl, sl] + np.outer(mup, mup)
            C = Sub[t - 1, sl, sl] + np.outer(mu, mup)
            W = C - A @ Sp
            M = Sc - C @ A.T - A @ W.T
            L = _cholesky(Q)
            GQ = _cotangent(L, M)
            GA = _solve_upper(L.T, _solve_lower(L, W))
            X = GQ @ A
            contract(GA - 2 * X @ P, GQ - A.T @ X, a, p, dt)
    return out


def leaves_from_score(spec, score):
    """Flat leaf gradients (the order of flat_params) from a [nterm, 3, 2] score."""
    out = []
    for c, term in enumerate(terms_of(spec)):
        for f, leaf in enumerate(term):
            out.extend(leaf_grads(leaf, score[c, f, 0], score[c, f, 1]))
    return np.array(out)


# -- posterior pairwise moments of the oracle -------------------------------------------------------------------------------------------------
def oracle_moments(spec, jitter, t, y, noise_var):
    """(x, Sig, Sub) of one chain from oracle.np_kalman's posterior state-space model: x = posterior mean - prior mean."""
    k = build_np(spec, jitter)
    prior = k.state_space_model(t)
    kf = np_kalman.KalmanFilter(prior, k.emission_matrix(t), y[:, None], np.array([[np.sqrt(noise_var)]]))
    post = kf.posterior_state_space_model()
    Sig, Sub = post.covariance_blocks()
    return post.marginal_means - prior.marginal_means, Sig, Sub


# -- (i): the dense oracle --------------------------------------------------------------------------------------------------------------------
def k_closed(spec, r):
    """k(r) in closed form, hyper-parameters of any scalar type (complex for the complex step), r real >= 0."""
    k = spec[0]
    if k == "M12":
        return spec[2] * np.exp(-r / spec[1])
    if k == "OU":
        return spec[2] / (2.0 * spec[1]) * np.exp(-spec[1] * r)
    if k == "M32":
        z = np.sqrt(3.0) * r / spec[1]
        return spec[2] * (1.0 + z) * np.exp(-z)
    if k == "M52":
        z = np.sqrt(5.0) * r / spec[1]
        return spec[2] * (1.0 + z + z * z / 3.0) * np.exp(-z)
    if k == "H":
        return spec[1] * np.cos(2.0 * np.pi * r / spec[2])
    if k == "C":
        return spec[1] * np.ones_like(r)
    parts = [k_closed(c, r) for c in spec[1]]
    out = parts[0]
    for p in parts[1:]:
        out = out + p if k == "Sum" else out * p
    return out


def k_ssm(spec, jitter, t, dtype):
    """The f-covariance of the state-space prior on the sorted points t, jitter included (P0 = Pinf + jitter I, Q + jitter I), from
    term_blocks in `dtype` (complex for the complex step)."""
    terms = terms_of(spec)
    T = len(t)
    K = np.zeros((T, T), dtype=dtype)
    for term in terms:
        n = int(np.prod([LEAF_DIM[f[0]] for f in term]))
        H = kron_all([np.eye(1, LEAF_DIM[f[0]]) for f in term])
        eye = np.eye(n)
        S, As = [], []
        for i in range(T):
            if i == 0:
                S.append(term_blocks(term, 0.0, dtype)[1] + jitter * eye)
                continue
            A, _, Q, _, _ = term_blocks(term, t[i] - t[i - 1], dtype)
            As.append(A)
            Qj = Q + jitter * eye if (Q + jitter * eye).any() else Q
            S.append(A @ S[-1] @ A.T + Qj)
        for j in range(T):
            Cj = S[j]
            K[j, j] += (H @ Cj @ H.T)[0, 0]
            for i in range(j + 1, T):
                Cj = As[i - 1] @ Cj
                K[i, j] += (H @ Cj @ H.T)[0, 0]
                K[j, i] = K[i, j]
    return K


def dense_ll_and_grad(spec, jitter, t, y, noise_var):
    """(ll, flat kernel gradients, d ll / d noise_var) of one chain from the dense K + noise_var I."""
    T = len(t)
    r = np.abs(t[:, None] - t[None, :])
    kfun = (lambda s, dtype: k_closed(s, r).astype(dtype)) if jitter == 0.0 else (lambda s, dtype: k_ssm(s, jitter, t, dtype))
    K = kfun(spec, np.float64) + noise_var * np.eye(T)
    L = np.linalg.cholesky(K)
    alpha = np.linalg.solve(L.T, np.linalg.solve(L, y))
    ll = -0.5 * y @ alpha - np.log(np.diag(L)).sum() - 0.5 * T * np.log(2 * np.pi)
    Li = np.linalg.solve(L, np.eye(T))
    Wm = np.outer(alpha, alpha) - Li.T @ Li
    params = flat_params(spec)
    grads = []
    for i in range(len(params)):
        step = [complex(p, 1e-30 if j == i else 0.0) for j, p in enumerate(params)]
        dK = kfun(with_params(spec, step), complex).imag / 1e-30
        grads.append(0.5 * (Wm * dK).sum())
    return ll, np.array(grads), 0.5 * np.trace(Wm)


# -- the trees of the tests: (name, tree, jitter), state dimensions 1 .. 8 and every shape of term the kernel instantiates -------------------
M12, OU, M32, M52 = ("M12", 1.3, 0.8), ("OU", 0.9, 1.1), ("M32", 1.3, 0.8), ("M52", 1.3, 0.8)
HARM, HARM2, CONST = ("H", 1.1, 2.5), ("H", 0.9, 1.7), ("C", 0.6)
TREES = [
    ("matern12", M12, 0.0),
    ("ou", OU, 0.0),
    ("matern32", M32, 0.0),
    ("matern52", M52, 0.0),
    ("sum_m32_m12", ("Sum", [M32, ("M12", 0.7, 1.2)]), 0.0),
    ("sum_m52_m32", ("Sum", [M52, ("M32", 0.9, 0.5)]), 0.0),
    ("prod_m32_h", ("Prod", [M32, HARM]), 0.0),
    ("prod_m52_h", ("Prod", [M52, HARM]), 0.0),
    ("sum_m52_m32_m32", ("Sum", [M52, ("M32", 0.9, 0.5), ("M32", 2.1, 1.4)]), 0.0),
    ("sum_m52_m52_m32", ("Sum", [M52, ("M52", 0.8, 0.6), ("M32", 2.1, 1.4)]), 0.0),
    ("prod_m32_h_h", ("Prod", [M32, HARM, HARM2]), 0.0),
    ("sum_prod_m12_h_const", ("Sum", [("Prod", [M12, HARM]), CONST]), 1e-6),
    ("const_jitter", CONST, 1e-3),
]


def make_grid(rng, spec, T, min_gap=0.5, zeros=0):
    """Sorted points with gaps max(Exp(0.5 l), min_gap l), l the tree's shortest time scale (1 for a Constant), `zeros` of the gaps
    set to exactly zero."""
    lm = shortest_lengthscale(spec)
    lm = 1.0 if not np.isfinite(lm) else lm
    gaps = np.maximum(rng.exponential(0.5 * lm, T - 1), min_gap * lm)
    if zeros:
        gaps[rng.choice(T - 1, size=zeros, replace=False)] = 0.0
    return np.concatenate([[0.0], np.cumsum(gaps)])


# Worst fp64-against-long-double spread of score_restatement over TREES on the grids of tests/test_host_hyper.py (T = 40, the conftest
# seed), relative to max(1, |g|): measured there (test_fp64_against_long_double prints and bounds every tree's value); the GPU tests
# allow 10 x this.
FP64_SPREAD = 6.6e-12      # measured 6.52e-12 (sum_m52_m52_m32); <= 3.4e-13 for the trees without a Sum of Matern-5/2
