"""
numpy fp64 closed form of the joint posterior covariance (include/scfgp_hip.h: scfgp_predict_cov): under w ~ N(alpha, kappa A^-1),
A^-1 = Li^T Li,

    Cov[f(a_i), f(b_j)] = kappa phi(a_i)^T A^-1 phi(b_j) = kappa (Phi_a Li^T)(Phi_b Li^T)^T

with the oracle's feature map; `noise` adds kappa to the diagonal of the symmetric form.
"""
import numpy as np

from oracle import scfgp_oracle as O


def kappa(params):
    return float(np.log1p(np.exp(params[2])))


def factor(X, Li, params, S, M):
    """C = Phi(X) Li^T (T, K); entries of Li above the diagonal are not read."""
    X = np.asarray(X, np.float64)
    return O.feature_map(X, params, X.shape[1], S, M) @ np.tril(np.asarray(Li, np.float64)).T


def pred_cov(Xa, Li, params, S, M, Xb=None, noise=False):
    """(Ta, Tb) covariance at the scaled rows Xa, Xb (None: among the rows of Xa, + kappa on the diagonal with noise)."""
    if Xb is not None and noise:
        raise ValueError('noise is defined for the symmetric form only')
    kap = kappa(params)
    Ca = factor(Xa, Li, params, S, M)
    Cb = Ca if Xb is None else factor(Xb, Li, params, S, M)
    cov = kap * (Ca @ Cb.T)
    if noise:
        cov[np.diag_indices_from(cov)] += kap
    return cov
