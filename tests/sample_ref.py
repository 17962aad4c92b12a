"""
numpy restatement of the posterior sample functions (include/scfgp_hip.h: scfgp_sample, scfgp_sample_weights), vectorised:

    Philox4x64-10 (Random123), counter (c0, c1, 0, 0), key (seed, stream); U(u) = ((u >> 11) + 0.5) 2^-53
    normal of sample s from the block's words w, p = (s & 3) >> 1:  r = sqrt(-2 ln U(w[2p])),  r cos(2 pi U(w[2p+1])) (s even) / r sin (s odd)
    z[k][s] = normal of block (k, s >> 2), stream 0;   eps[t][s] = normal of block (t, s >> 2), stream 1
    W = alpha 1^T + sqrt(kappa) Li^T Z,   f = Phi* W,   y = f + sqrt(kappa) eps
"""
import numpy as np

from oracle import scfgp_oracle as O

_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
PHILOX_M = (np.uint64(0xD2E7470EE14C6C93), np.uint64(0xCA5A826395121157))
PHILOX_W = (np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBB67AE8584CAA73B))


def _mulhilo(a, b):
    """(hi, lo) 64-bit halves of the 128-bit products a * b, element-wise on uint64 arrays"""
    a0, a1 = a & _M32, a >> _S32
    b0, b1 = b & _M32, b >> _S32
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (p00 >> _S32) + (p01 & _M32) + (p10 & _M32)
    hi = p11 + (p01 >> _S32) + (p10 >> _S32) + (mid >> _S32)
    return hi, a * b


def philox4x64_10(c0, c1, c2, c3, k0, k1):
    """Philox4x64-10 of counters (c0, c1, c2, c3) and keys (k0, k1), broadcast element-wise; returns the four output words."""
    c = [np.asarray(x, dtype=np.uint64) for x in np.broadcast_arrays(c0, c1, c2, c3, k0, k1)]
    c0, c1, c2, c3, k0, k1 = [x.copy() for x in c]
    with np.errstate(over='ignore'):
        for r in range(10):
            if r:
                k0 = k0 + PHILOX_W[0]
                k1 = k1 + PHILOX_W[1]
            hi0, lo0 = _mulhilo(PHILOX_M[0], c0)
            hi1, lo1 = _mulhilo(PHILOX_M[1], c2)
            c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
    return c0, c1, c2, c3


def u01(u):
    return ((np.asarray(u, dtype=np.uint64) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def normals(idx, nsamp, seed, stream):
    """(len(idx), nsamp) standard normals: element [i][s] of index idx[i] (k or t), sample s, stream 0 (weights) / 1 (noise)."""
    idx = np.asarray(idx, dtype=np.uint64).reshape(-1, 1)
    s = np.arange(nsamp)
    w = philox4x64_10(idx, (s >> 2).astype(np.uint64)[None, :], 0, 0, np.uint64(seed), np.uint64(stream))
    hi = (s & 2) != 0
    a = np.where(hi, w[2], w[0])
    b = np.where(hi, w[3], w[1])
    r = np.sqrt(-2.0 * np.log(u01(a)))
    th = 2.0 * np.pi * u01(b)
    return np.where((s & 1) != 0, r * np.sin(th), r * np.cos(th))


def kappa(params):
    return float(np.log1p(np.exp(params[2])))


def weights(alpha, Li, kap, nsamp, seed):
    """W (K, nsamp) = alpha 1^T + sqrt(kappa) Li^T Z."""
    alpha = np.asarray(alpha, np.float64).reshape(-1)
    Li = np.tril(np.asarray(Li, np.float64))
    Z = normals(np.arange(alpha.size), nsamp, seed, 0)
    return alpha[:, None] + np.sqrt(kap) * (Li.T @ Z)


def samples(Xs, alpha, Li, params, S, M, nsamp, seed, noise=False, t0=0):
    """(T, nsamp) sample functions at the scaled rows Xs (row t has index t0 + t in the call), with observation noise if asked."""
    Xs = np.asarray(Xs, np.float64)
    kap = kappa(params)
    f = O.feature_map(Xs, params, Xs.shape[1], S, M) @ weights(alpha, Li, kap, nsamp, seed)
    if noise:
        f = f + np.sqrt(kap) * normals(t0 + np.arange(Xs.shape[0]), nsamp, seed, 1)
    return f
