"""
numpy fp64 references of the partial-dependence (PD) and ICE curves of single inputs (include/scfgp_hip.h: scfgp_predict_pd) on the
oracle's feature map.  Pool rows x_t, weights w_t, W = sum w_t, a dimension d with grid values g_i; x_t^{d->g} is row t with column d
replaced by g:

    ice[t][i] = phi(x_t^{d->g_i}) . alpha         pd[i] = sum_t (w_t / W) ice[t][i] = Phibar[i] . alpha
    Phibar[i] = sum_t (w_t / W) phi(x_t^{d->g_i})  cov = kappa Phibar A^-1 Phibar^T = kappa (Phibar Li^T)(Phibar Li^T)^T,  sd = sqrt(diag)

brute() expands every (row, grid value) pair and goes through the oracle's feature map.  closed() is the form the device runs: the
features phi0 at the rows with column d cleared, rotated pair by pair by g_i Fall[d][j]; only the weighted mean of phi0 enters the PD
curve.  `mutate` breaks the closed form on purpose (tests/test_pd_ref.py: the parity bounds can tell the forms apart).
"""
import numpy as np

from oracle import scfgp_oracle as O
from tests import gradcov_ref as GR
from tests.pred_grad_ref import fall

MUTATIONS = ('wrong_sign', 'swap_halves', 'no_kappa', 'unnormalised_w')
GEOMETRIES = GR.GEOMETRIES
synthetic = GR.synthetic
points = GR.points
kappa = GR.kappa


def dims_for(D):
    """the dimensions the GPU tier asks for: all of them up to D = 16, else the two ends and the middle"""
    return list(range(D)) if D <= 16 else [0, D // 2, D - 1]


def make_grid(Xs, dims, G, seed=0):
    """ndim x G grid values inside (and a little outside) the range of the rows' own columns, not sorted"""
    rng = np.random.default_rng(0x9D + seed)
    Xs = np.asarray(Xs, np.float64)
    lo, hi = Xs[:, dims].min(0), Xs[:, dims].max(0)
    span = np.where(hi > lo, hi - lo, 1.0)
    return (lo - 0.1 * span)[:, None] + rng.uniform(0, 1.2, (len(dims), G)) * span[:, None]


def _weights(w, T):
    return np.ones(T) if w is None else np.asarray(w, np.float64).reshape(-1)


def _posterior(Phibar, alpha, Li, kap):
    C = Phibar @ np.tril(np.asarray(Li, np.float64)).T
    cov = kap * (C @ C.T)
    return Phibar @ alpha, np.sqrt(np.einsum('ik,ik->i', C, C) * kap), cov


def brute(Xs, w, alpha, Li, params, S, M, dims, grid, want_ice=True):
    """pd (ndim, G), sd (ndim, G), cov (ndim, G, G), ice (ndim, T, G) or None, and the mean feature rows Phibar (ndim, G, K), by
    expanded rows through the oracle's feature map.  Rows of weight 0 are left out of the sums (they may hold anything)."""
    Xs = np.asarray(Xs, np.float64)
    T, D = Xs.shape
    w = _weights(w, T)
    live = w > 0
    alpha = np.asarray(alpha, np.float64).reshape(-1)
    grid = np.asarray(grid, np.float64)
    nd, G = grid.shape
    K = 2 * (S + M)
    pd = np.empty((nd, G)); sd = np.empty((nd, G)); cov = np.empty((nd, G, G)); Pb = np.empty((nd, G, K))
    ice = np.empty((nd, T, G)) if want_ice else None
    wl = w[live] / w[live].sum()
    for a, d in enumerate(dims):
        mu_mean = np.empty(G)
        for i in range(G):
            Xe = Xs.copy(); Xe[:, d] = grid[a, i]
            Phi = O.feature_map(Xe, params, D, S, M)
            mu = Phi @ alpha
            if want_ice:
                ice[a, :, i] = mu
            mu_mean[i] = wl @ mu[live]
            Pb[a, i] = wl @ Phi[live]
        _, sd[a], cov[a] = _posterior(Pb[a], alpha, Li, kappa(params))
        pd[a] = mu_mean
    return pd, sd, cov, ice, Pb


def closed(Xs, w, alpha, Li, params, S, M, dims, grid, mutate=None, want_ice=True):
    """the same numbers by the rotation of the zeroed-column features"""
    Xs = np.asarray(Xs, np.float64)
    T, D = Xs.shape
    J = S + M
    w = _weights(w, T)
    live = w > 0
    what = w[live] if mutate == 'unnormalised_w' else w[live] / w[live].sum()
    alpha = np.asarray(alpha, np.float64).reshape(-1)
    ac, as_ = alpha[:J], alpha[J:]
    grid = np.asarray(grid, np.float64)
    nd, G = grid.shape
    Om = fall(params, D, S, M)                                    # D x J
    kap = 1.0 if mutate == 'no_kappa' else kappa(params)
    pd = np.empty((nd, G)); sd = np.empty((nd, G)); cov = np.empty((nd, G, G)); Pb = np.empty((nd, G, 2 * J))
    ice = np.empty((nd, T, G)) if want_ice else None
    for a, d in enumerate(dims):
        X0 = Xs.copy(); X0[:, d] = 0.0
        Phi0 = O.feature_map(X0, params, D, S, M)
        if mutate == 'swap_halves':
            Phi0 = np.concatenate((Phi0[:, J:], Phi0[:, :J]), 1)
        th = grid[a][:, None] * Om[d][None, :]                    # G x J
        c, s = np.cos(th), np.sin(th)
        if mutate == 'wrong_sign':
            s = -s
        if want_ice:
            R = np.concatenate((ac[None, :] * c + as_[None, :] * s, as_[None, :] * c - ac[None, :] * s), 1).T      # K x G
            ice[a] = Phi0 @ R
        m0 = what @ Phi0[live]
        mc, ms = m0[:J], m0[J:]
        Pb[a] = np.concatenate((mc[None, :] * c - ms[None, :] * s, ms[None, :] * c + mc[None, :] * s), 1)
        pd[a], sd[a], cov[a] = _posterior(Pb[a], alpha, Li, kap)
    return pd, sd, cov, ice, Pb


def cancellation(Xs, w, params, S, M, dims):
    """min over the dimensions of |phibar0| / |phi|: how much of a feature row's norm survives the averaging (an input condition of the
    tests: pd then suffers no catastrophic cancellation)"""
    Xs = np.asarray(Xs, np.float64)
    T, D = Xs.shape
    w = _weights(w, T)
    out = np.inf
    for d in dims:
        X0 = Xs.copy(); X0[:, d] = 0.0
        Phi0 = O.feature_map(X0[w > 0], params, D, S, M)
        out = min(out, np.linalg.norm((w[w > 0] / w.sum()) @ Phi0) / np.linalg.norm(Phi0[0]))
    return float(out)
