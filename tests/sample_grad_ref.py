"""
fp64 numpy reference of scfgp_sample_grad (include/scfgp_hip.h): values and input gradients of posterior sample functions, one sample
per row.  With Phi = s [cos Z | sin Z], Z = Xs Fall + offsets (tests/pred_grad_ref.py) and W (K, nsamp) the weights of
tests/sample_ref.py, column s = [w_c | w_s] in alpha's layout:

    f_t        = sum_j phi_c_tj W[j][s_t] + phi_s_tj W[J + j][s_t],            s_t = sidx[t]  (None: t % nsamp)
    d f_t / d x_d = sum_j Fall[d][j] (phi_c_tj W[J + j][s_t] - phi_s_tj W[j][s_t])
"""
import numpy as np

from oracle import scfgp_oracle as O
from tests import pred_grad_ref as G


def default_sidx(T, nsamp):
    return np.arange(T, dtype=np.int64) % int(nsamp)


def sample_grad(Xs, W, sidx, params, S, M):
    """val (T,), grad (T, D) of f_{sidx[t]} at the scaled rows Xs."""
    Xs = np.asarray(Xs, np.float64)
    W = np.asarray(W, np.float64)
    T, D = Xs.shape
    J = S + M
    sidx = default_sidx(T, W.shape[1]) if sidx is None else np.asarray(sidx, np.int64)
    Phi = O.feature_map(Xs, params, D, S, M)
    pc, ps = Phi[:, :J], Phi[:, J:]
    Wr = W.T[sidx]                                     # (T, K): the weight vector of each row
    wc, ws = Wr[:, :J], Wr[:, J:]
    val = (pc * wc + ps * ws).sum(1)
    grad = (pc * ws - ps * wc) @ G.fall(params, D, S, M).T
    return val, grad


def projected_gradient_norm(X, grad, lo, hi, minimize=False):
    """Norm of the gradient of an ascent (minimize: descent) step with the components that push out of the box [lo, hi] at an active
    bound removed: zero exactly at the stationary points of the box-constrained problem."""
    g = -np.asarray(grad) if minimize else np.asarray(grad)
    g = np.where((X <= lo) & (g < 0), 0.0, g)
    g = np.where((X >= hi) & (g > 0), 0.0, g)
    return np.sqrt((g ** 2).sum(1))
