"""
numpy fp64 closed form of the posterior distribution of the input gradient (include/scfgp_hip.h: scfgp_predict_gradcov) on the
oracle's feature map.  Under w ~ N(alpha, kappa A^-1), A^-1 = Li^T Li, the gradient grad f(x) = J(x)^T w is Gaussian:

    J(x) (K x D): J[k][d] = phi'_k(x) Fall2[d][k],   phi' = (-phi_s | phi_c),   Fall2 = [Fall | Fall]  (both halves share the phases)
    m(x) = J(x)^T alpha = grad mu*,        Sigma(x) = kappa J(x)^T A^-1 J(x) = kappa (Li J)^T (Li J)      (no noise term)
    raw X:  m -> g o m,  Sigma -> diag(g) Sigma diag(g),  g = d forward_transform / d x at the raw input
    asub = sum_t w_t (m_t m_t^T + Sigma_t) / sum_t w_t

gradcov() is dense over Fall with no latent shortcut; gradcov_latent() is the form the device runs (q = min(D, S) directions per
point).  `mutate` breaks the closed form on purpose (tests/test_gradcov_ref.py: the parity bounds can tell the forms apart).
"""
import numpy as np

from oracle import scfgp_oracle as O
from scfgp_amd import synth
from tests.pred_grad_ref import fall

MUTATIONS = ('no_minus', 'swap_halves', 'no_kappa', 'one_sided_g')

# (D, S, M) of the GPU tier (tests/test_gpu_predict_gradcov.py) and what each covers
GEOMETRIES = [(1, 2, 2), (7, 12, 3), (70, 5, 60), (15, 15, 60), (16, 16, 70), (40, 33, 20), (64, 64, 8), (65, 64, 8)]


def kappa(params):
    return float(np.log1p(np.exp(params[2])))


def synthetic(D, S, M):
    """parameters, alpha and the synthetic Li of tests/test_gpu_predict_cov.py: the inputs of the GPU tier, reproducible on the CPU"""
    seed = 0x5CF65000 + M
    K = 2 * (S + M)
    params = synth.make_params(seed + 0x0202, D, S, M, abc=(-1.0, 0.0, -1.0))
    rng = np.random.default_rng(seed)
    alpha = rng.standard_normal(K) / np.sqrt(K)
    Li = np.tril(rng.standard_normal((K, K))) / np.sqrt(K)
    return params, alpha, Li


def points(D, T=257):
    """the T scaled rows the GPU tier evaluates a geometry at"""
    return synth.make_X(0x6AD + D, T, D)


def raw_problem(xalgo, N=600, T=50, seed=5):
    """raw mode of the GPU tier: 4 raw columns, one of them constant (dropped by the scaler), the fitted X scaler, the synthetic
    factors at (D, S, M) = (3, 2, 40) and T raw rows"""
    from scfgp_amd.scaler import Scaler
    rng = np.random.default_rng(seed)
    Xr = np.column_stack([rng.uniform(0.5, 3.0, N + T), rng.gamma(2.0, 1.0, N + T), np.full(N + T, 2.5), rng.normal(1.0, 2.0, N + T)])
    xs = Scaler(xalgo); xs.fit(Xr[:N])
    D, S, M = 3, 2, 40
    return (D, S, M), xs, synthetic(D, S, M), Xr[N:]


def dphi(Xs, params, S, M, mutate=None):
    """phi'(x) (T x K): the derivative of every feature in its own phase"""
    Xs = np.asarray(Xs, np.float64)
    J = S + M
    Phi = O.feature_map(Xs, params, Xs.shape[1], S, M)
    pc, ps = Phi[:, :J], Phi[:, J:]
    if mutate == 'no_minus':
        return np.concatenate((ps, pc), 1)
    if mutate == 'swap_halves':
        return np.concatenate((pc, -ps), 1)
    return np.concatenate((-ps, pc), 1)


def jacobian(Xs, params, S, M, mutate=None):
    """J (T x K x D): d phi_k / d x_d at every row"""
    D = np.asarray(Xs).shape[1]
    Fa = fall(params, D, S, M)                                    # D x J
    return dphi(Xs, params, S, M, mutate)[:, :, None] * np.concatenate((Fa, Fa), 1).T[None, :, :]


def _chain(m, Sig, g, mutate):
    if g is None:
        return m, Sig
    g = np.asarray(g, np.float64)
    Sig = Sig * g[:, :, None] if mutate == 'one_sided_g' else Sig * g[:, :, None] * g[:, None, :]
    return m * g, Sig


def gradcov(Xs, alpha, Li, params, S, M, g=None, mutate=None):
    """m (T, D), Sigma (T, D, D) at the scaled rows Xs; g (T, D): the X scaler's derivative factors of raw mode"""
    Jx = jacobian(Xs, params, S, M, mutate)
    m = np.einsum('tkd,k->td', Jx, np.asarray(alpha, np.float64).reshape(-1))
    G = np.tril(np.asarray(Li, np.float64)) @ Jx                                    # Li J_t (T x K x D)
    Sig = (1.0 if mutate == 'no_kappa' else kappa(params)) * (G.transpose(0, 2, 1) @ G)
    return _chain(m, Sig, g, mutate)


def basis(params, D, S, M):
    """Q (J x q), P (D x q) with Fall[d][j] = sum_i P[d][i] Q[j][i], q = min(D, S)"""
    _, _, _, l_F, r_F, F, _, _ = O.unpack_params(params, D, S, M)
    if D <= S:
        return np.concatenate((l_F, F), 1).T.copy(), np.eye(D)
    return np.concatenate((np.eye(S), r_F.T), 1).T.copy(), l_F


def gradcov_latent(Xs, alpha, Li, params, S, M, g=None):
    """the same numbers in the form of the device: Psi_t (q x K), C'_t = Psi_t Li^T, H_t = C'_t C'_t^T, Sigma_t = kappa P H_t P^T"""
    D = np.asarray(Xs).shape[1]
    Q, P = basis(params, D, S, M)
    Psi = dphi(Xs, params, S, M)[:, None, :] * np.concatenate((Q, Q), 0).T[None, :, :]           # T x q x K
    C = Psi @ np.tril(np.asarray(Li, np.float64)).T
    H = C @ C.transpose(0, 2, 1)
    m = (Psi @ np.asarray(alpha, np.float64).reshape(-1)) @ P.T
    return _chain(m, kappa(params) * (P @ H @ P.T), g, None)


def asub(m, Sig, w=None):
    """sum_t w_t (m_t m_t^T + Sigma_t) / sum_t w_t"""
    w = np.ones(m.shape[0]) if w is None else np.asarray(w, np.float64).reshape(-1)
    return np.einsum('t,tde->de', w, m[:, :, None] * m[:, None, :] + Sig) / w.sum()
