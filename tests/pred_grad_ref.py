"""
fp64 numpy reference of the input gradients of pred_func (SCFGP/SCFGP.py:138-148) and of the scalers' chain rules
(SCFGP/Scaler.py forward / backward transforms) -- the closed forms scfgp_predict_grad implements:

    Phi = s [cos Z | sin Z], Z = Xs Fall + offsets, alpha = [alpha_c | alpha_s], V = Phi Li^T Li
    d mu / d x_d    = sum_j Fall[d][j] (phi_c alpha_s - phi_s alpha_c)_j
    d sigma / d x_d = kappa / sigma * sum_j Fall[d][j] (phi_c V_s - phi_s V_c)_j,   sigma = sqrt(kappa (1 + ||Li phi||^2))
"""
import numpy as np
from scipy.stats import norm

from oracle import scfgp_oracle as O


def fall(params, D, S, M):
    """[l_F | F] (D x J): the x-part of the phase projection (SCFGP.py:139-140)."""
    _, _, _, l_F, _, F, _, _ = O.unpack_params(params, D, S, M)
    return np.concatenate((l_F, F), 1)


def predict_grad(Xs, alpha, Li, params, S, M):
    """mu (T,1), std (T,), dmu (T,D), dstd (T,D) of pred_func at Xs."""
    Xs = np.asarray(Xs, np.float64)
    D = Xs.shape[1]
    J = S + M
    Phi = O.feature_map(Xs, params, D, S, M)
    pc, ps = Phi[:, :J], Phi[:, J:]
    al = np.asarray(alpha, np.float64).reshape(-1)
    Li = np.asarray(Li, np.float64)
    Fa = fall(params, D, S, M)
    kappa = np.log1p(np.exp(params[2]))
    C = Phi @ Li.T
    sd = np.sqrt(kappa * (1 + (C ** 2).sum(1)))
    V = C @ Li
    dmu = (pc * al[J:] - ps * al[:J]) @ Fa.T
    dsd = (kappa / sd)[:, None] * ((pc * V[:, J:] - ps * V[:, :J]) @ Fa.T)
    return Phi @ al[:, None], sd, dmu, dsd


def x_scaler_deriv(scaler, X_raw):
    """d forward_transform / d x, column by column (T x len(cols)) at the raw rows X_raw (all columns)."""
    d = scaler.data
    x = np.asarray(X_raw, np.float64)[:, d['cols']]
    a = scaler.algo
    if a == 'min-max':
        return np.broadcast_to(1.0 / (d['max'] - d['min']), x.shape).copy()
    if a == 'normal':
        return np.broadcast_to(1.0 / d['std'], x.shape).copy()
    if a == 'inv-normal':
        return norm.pdf((x - d['mu']) / d['std']) / d['std']
    t = (x - d['min']) / (d['max'] - d['min'])
    lm = d['boxcox'][None, :]
    bc = (np.sign(t) * np.abs(t) ** lm - 1) / lm
    dz = np.abs(t) ** (lm - 1) / ((d['max'] - d['min']) * d['std'])
    return dz if a == 'auto-normal' else norm.pdf((bc - d['mu']) / d['std']) * dz


def y_backward_deriv(scaler, x):
    """d backward_transform / d x of a single-column scaler, element-wise."""
    d = scaler.data
    g = lambda k: float(np.asarray(d[k]).reshape(-1)[0])
    x = np.asarray(x, np.float64)
    a = scaler.algo
    if a == 'min-max':
        return np.full_like(x, g('max') - g('min'))
    if a == 'normal':
        return np.full_like(x, g('std'))
    if a == 'inv-normal':
        return 1.0 / (norm.pdf(norm.ppf(x)) * g('std'))
    if a == 'auto-normal':
        t, dt = x * g('std') + g('mu'), g('std')
    else:
        z = norm.ppf(x)
        t, dt = z * g('std') + g('mu'), g('std') / norm.pdf(z)
    lm = g('boxcox')
    return (g('max') - g('min')) * np.abs(t * lm + 1) ** (1 / lm - 1) * dt


def y_chain(scaler, mu, sd, dmu, dsd):
    """Gradients of mu_y = bw(mu), std_y = (bw(mu + sd) - bw(mu - sd)) / 2 from those of mu (T,1 or T), sd (T) -- SCFGP.py:281-284."""
    mu = np.asarray(mu).reshape(-1, 1); sd = np.asarray(sd).reshape(-1, 1)
    bp, bm = y_backward_deriv(scaler, mu + sd), y_backward_deriv(scaler, mu - sd)
    return y_backward_deriv(scaler, mu) * dmu, 0.5 * (bp * (dmu + dsd) - bm * (dmu - dsd))
