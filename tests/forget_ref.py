"""
numpy fp64 form of the posterior downdate (include/scfgp_hip.h: scfgp_forget): with a fit A = Phi^T Phi + lam I = L L^T, Li = L^-1,
alpha = A^-1 Phi^T y and n of ITS rows (Xo, yo) with the oracle's features Phi_o at the same hyper-parameters,

    C = Phi_o Li^T,  r = yo - Phi_o alpha,  S = I - C^T C = M M^T,  Li' = M^-1 Li,  gamma = S^-1 C^T r,  alpha' = alpha - Li^T gamma

A' = A - Phi_o^T Phi_o = (L M)(L M)^T with L M lower triangular and a positive diagonal, so (alpha', Li') are the factors of the fit on
the remaining rows.  The held-out predictions of the removed rows are the oracle's predict with (alpha', Li'), and

    log p(yo | rest) = -1/2 [ (r^T r + |M^-1 C^T r|^2) / kappa + n log(2 pi kappa) - 2 sum_i log M_ii ]
"""
import numpy as np

from oracle import scfgp_oracle as O


def kappa(params):
    return float(np.log1p(np.exp(params[2])))


def forget(Xo, yo, alpha, Li, params, S, M, C_model=None):
    """dict(alpha (K,1), Li (K,K), mu (n,), std (n,), stats (8,), lam_min: the smallest eigenvalue of S) from scaled rows Xo (n,D) and
    scaled targets yo (n,) or (n,1) that are in the fit (alpha, Li); entries of Li above the diagonal are not read.  numpy raises
    LinAlgError where S has no Cholesky factor.  C_model(Phi, Li^T): the C that C^T C and C^T r are formed from in place of the fp64
    product (e.g. tests/parity.apply32_model: the C an fp32 context holds)."""
    Xo = np.asarray(Xo, np.float64); yo = np.asarray(yo, np.float64).reshape(-1, 1)
    n = Xo.shape[0]
    Li = np.tril(np.asarray(Li, np.float64)); alpha = np.asarray(alpha, np.float64).reshape(-1, 1)
    Phi = O.feature_map(Xo, params, Xo.shape[1], S, M)
    C = Phi @ Li.T if C_model is None else np.asarray(C_model(Phi, Li.T), np.float64)
    r = yo - Phi @ alpha
    Sm = np.eye(Li.shape[0]) - C.T @ C
    Mc = np.linalg.cholesky(Sm)
    Li_new = np.tril(np.linalg.solve(Mc, Li))
    w = np.linalg.solve(Mc, C.T @ r)
    gamma = np.linalg.solve(Mc.T, w)
    alpha_new = alpha - Li.T @ gamma
    mu, sd = O.predict(Xo, alpha_new, Li_new, params, S, M)
    mu = np.asarray(mu).ravel(); sd = np.asarray(sd).ravel()
    kap = kappa(params)
    e = yo.ravel() - mu
    marg = -0.5 * (e ** 2 / sd ** 2 + np.log(2 * np.pi * sd ** 2))
    joint = -0.5 * (((r.T @ r).item() + (w.T @ w).item()) / kap + n * np.log(2 * np.pi * kap) - 2.0 * np.sum(np.log(np.diag(Mc))))
    stats = np.array([n, np.sum(e ** 2), np.sum(np.abs(e)), np.sum(marg), joint, np.min(np.diag(Mc)) ** 2, 1.0, 0.0])
    return dict(alpha=alpha_new, Li=Li_new, mu=mu, std=sd, stats=stats, lam_min=float(np.linalg.eigvalsh(Sm)[0]))


def tiled_row(X, y, alpha, Li, params, S, M, i=0):
    """(Xo, yo, k, h): row i of the fit repeated k times with k h >= 2 (h its leverage), so that S = I - k c c^T has the eigenvalue
    1 - k h <= -1 and no Cholesky factor"""
    c = O.feature_map(np.asarray(X[i:i + 1], np.float64), params, X.shape[1], S, M) @ np.tril(np.asarray(Li, np.float64)).T
    h = (c @ c.T).item()
    k = int(np.ceil(2.0 / h))
    return np.repeat(np.asarray(X[i:i + 1]), k, axis=0), np.repeat(np.asarray(y).reshape(-1)[i:i + 1], k), k, h
