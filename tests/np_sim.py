"""NumPy restatement of the simulation contract of include/mfgm.h: Philox4x32-10, the uniforms and Box-Muller of the normal stream, and
the Euler-Maruyama recursion with the reference's time alignment (markovflow/sde/sde_utils.py:36-96)."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: 4 arrays (broadcastable) of uint32 words, key: 2 words -> the 4 output words (uint32 arrays)."""
    c = [np.asarray(w, dtype=np.uint64) & _MASK for w in ctr]
    c = np.broadcast_arrays(*c)
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & _MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & _MASK
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0 = (k0 + np.uint64(W0)) & _MASK
        k1 = (k1 + np.uint64(W1)) & _MASK
    return [w.astype(np.uint32) for w in c]


def uniform53(lo, hi):
    n = (np.asarray(hi, dtype=np.uint64) << np.uint64(21)) | (np.asarray(lo, dtype=np.uint64) >> np.uint64(11))
    return (n.astype(np.float64) + 0.5) * 2.0 ** -53


def normals(seed, s, paths, steps, d):
    """z [len(paths), len(steps), d] of the stream `s` for the given path and step indices."""
    paths = np.asarray(paths, dtype=np.uint64)[:, None, None]
    steps = np.asarray(steps, dtype=np.uint64)[None, :, None]
    j = np.arange((d + 1) // 2, dtype=np.uint64)[None, None, :]
    w = philox4x32_10((j, steps, paths, np.uint64(s)), (seed & 0xFFFFFFFF, seed >> 32))
    u1, u2 = uniform53(w[0], w[1]), uniform53(w[2], w[3])
    r = np.sqrt(-2.0 * np.log(u1))
    z = np.stack([r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2)], axis=-1).reshape(len(paths.ravel()), len(steps.ravel()), -1)
    return z[..., :d]


def euler_maruyama(drift, x0, time_grid, L, z):
    """X [B, N, d] with X[:, 0] = x0, X[:, k+1] = X[:, k] + f(X[:, k]) dt_k + sqrt(dt_k) L z[:, k], dt_k = t_k - t_{k-1}, t_{-1} = 0."""
    x = np.array(x0, dtype=np.float64)
    tg = np.asarray(time_grid, dtype=np.float64)
    X = np.empty((x.shape[0], tg.shape[0], x.shape[1]))
    X[:, 0] = x
    tprev = 0.0
    for k in range(tg.shape[0] - 1):
        dt = tg[k] - tprev
        tprev = tg[k]
        x = x + drift(x) * dt + np.sqrt(dt) * (z[:, k] @ np.asarray(L).T)
        X[:, k + 1] = x
    return X
