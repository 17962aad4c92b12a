"""
numpy fp64 closed form of the posterior update by derivative observations (include/scfgp_hip.h: scfgp_condition_grad) on the oracle's
feature map.  grad f(x) = J(x)^T w is linear in the weights, so every observation is a row of a linear system in w:

    value of point t            phi_t                                                                 target  y_t
    d f / d x_d at point t      psi = sqrt(rho) g_t[d] (-phi_s o Fall[d, :] | phi_c o Fall[d, :])           target  sqrt(rho) G
    A = L L^T (L = Li^-1),  A' = A + Psi^T Psi,  alpha' = A'^-1 (A alpha + Psi^T t),  Li' = chol(A')^-1

rows() builds Psi and t literally, point by point; update() is the closed form above, which shares nothing with the device's
C / S / M route.  g (n x D): the X scaler's derivative factors of raw mode (Scaler.forward_derivative).  `mutate` breaks the rows on
purpose (tests/test_condition_grad_ref.py: the GPU tier's bounds can tell the forms apart).
"""
import numpy as np
from scipy.linalg import solve_triangular

from oracle import scfgp_oracle as O
from scfgp_amd import synth
from tests.pred_grad_ref import fall

MUTATIONS = ('no_minus', 'swap_halves', 'rho_on_row', 'no_sqrt_on_target', 'sorted_dims')
RAW_MUTATIONS = ('g_twice', 'no_g')
RHO_VALUES = (0.0, 0.25, 1.0, 100.0)

# (D, S, M, N0, n, dims) of the GPU tier (tests/test_gpu_condition_grad.py); dims None: all inputs in order
SHAPES = [(1, 2, 2, 60, 40, None), (5, 4, 60, 1000, 300, None), (5, 4, 60, 1000, 1, (3,)), (7, 12, 3, 200, 129, (6, 0, 3)),
          (70, 5, 60, 2000, 50, None), (16, 16, 70, 1500, 65, None), (64, 32, 1024, 4000, 16, None)]


def dphi(X, params, S, M, mutate=None):
    """phi'(x) (n x K), the derivative of every feature in its own phase: (-phi_s | phi_c)"""
    X = np.asarray(X, np.float64)
    J = S + M
    Phi = O.feature_map(X, params, X.shape[1], S, M)
    pc, ps = Phi[:, :J], Phi[:, J:]
    if mutate == 'no_minus':
        return np.concatenate((ps, pc), 1)
    if mutate == 'swap_halves':
        return np.concatenate((pc, -ps), 1)
    return np.concatenate((-ps, pc), 1)


def rows(X, params, S, M, G, dims=None, rho=None, y=None, g=None, mutate=None):
    """Psi (n nb x K) and its targets (n nb,), nb = nd + (1 with y): the block of point t is its value row, then its derivative rows in
    the order of dims"""
    X = np.asarray(X, np.float64)
    n, D = X.shape
    dims = list(range(D)) if dims is None else [int(d) for d in dims]
    if mutate == 'sorted_dims':
        dims = sorted(dims)
    G = np.asarray(G, np.float64).reshape(n, len(dims))
    rho = np.ones_like(G) if rho is None else np.asarray(rho, np.float64).reshape(G.shape)
    Fa = fall(params, D, S, M)
    F2 = np.concatenate((Fa, Fa), 1)                               # both halves share the phases
    Phi = O.feature_map(X, params, D, S, M)
    dP = dphi(X, params, S, M, mutate)
    Psi, tg = [], []
    for t in range(n):
        if y is not None:
            Psi.append(Phi[t]); tg.append(float(np.asarray(y).reshape(-1)[t]))
        for j, d in enumerate(dims):
            sr = np.sqrt(rho[t, j])
            gt = 1.0 if g is None else float(g[t, d])
            if mutate == 'g_twice':
                gt = gt * gt
            if mutate == 'no_g':
                gt = 1.0
            Psi.append((rho[t, j] if mutate == 'rho_on_row' else sr) * gt * dP[t] * F2[d])
            tg.append((1.0 if mutate == 'no_sqrt_on_target' and rho[t, j] > 0 else sr) * G[t, j])
    return np.array(Psi), np.array(tg)


def update(alpha, Li, Psi, tg):
    """(alpha' (K,1), Li' (K,K)) of A' = A + Psi^T Psi from the factors of A; entries of Li above the diagonal are not read"""
    Li = np.tril(np.asarray(Li, np.float64)); alpha = np.asarray(alpha, np.float64).reshape(-1, 1)
    K = Li.shape[0]
    L = solve_triangular(Li, np.eye(K), lower=True)
    A = L @ L.T
    A1 = A + Psi.T @ Psi
    L1 = np.linalg.cholesky(A1)
    rhs = A @ alpha + Psi.T @ np.asarray(tg, np.float64).reshape(-1, 1)
    a1 = solve_triangular(L1.T, solve_triangular(L1, rhs, lower=True), lower=False)
    return a1, np.tril(solve_triangular(L1, np.eye(K), lower=True))


def condition_grad(X, G, alpha, Li, params, S, M, dims=None, rho=None, y=None, g=None, mutate=None):
    Psi, tg = rows(X, params, S, M, G, dims, rho, y, g, mutate)
    return update(alpha, Li, Psi, tg)


def mean_grad(X, alpha, params, S, M):
    """the mean gradient J(x)^T alpha at the rows of X (n x D)"""
    X = np.asarray(X, np.float64)
    D = X.shape[1]
    Fa = fall(params, D, S, M)
    return (dphi(X, params, S, M) * np.asarray(alpha, np.float64).reshape(1, -1)) @ np.concatenate((Fa, Fa), 1).T


def unit_rho(params, D, S, M, dims=None):
    """rho_d = J / |Fall[d, :]|^2 per observed input: |phi|^2 = s^2 J and |psi_d|^2 = s^2 |Fall[d, :]|^2 exactly (every cos / sin pair has
    unit length), so this precision brings every derivative row to the length of a value row.  From F_all alone."""
    Fa = fall(params, D, S, M)
    dims = list(range(D)) if dims is None else list(dims)
    return np.array([Fa.shape[1] / float(Fa[d] @ Fa[d]) for d in dims])


def raw_problem(xalgo, yalgo='normal', seed=5, N=600, n=50):
    """raw mode: 4 raw columns, one of them constant (dropped by the scaler), targets y = exp(0.3 sin x0 + 0.1 x1) + noise with their
    analytic raw derivatives dY (n x 4; the entry of the constant column is arbitrary), the fitted scalers, parameters at (D, S, M) =
    (3, 2, 40) and the oracle's fit of the N scaled training rows"""
    from scfgp_amd.scaler import Scaler
    rng = np.random.default_rng(seed)
    Xr = np.column_stack([rng.uniform(0.5, 3.0, N + n), rng.gamma(2.0, 1.0, N + n), np.full(N + n, 2.5), rng.normal(1.0, 2.0, N + n)])
    f = np.exp(0.3 * np.sin(Xr[:, :1]) + 0.1 * Xr[:, 1:2])
    yr = f + 0.05 * rng.standard_normal((N + n, 1))
    dY = np.column_stack([f[:, 0] * 0.3 * np.cos(Xr[:, 0]), 0.1 * f[:, 0], np.full(N + n, 7.0), np.zeros(N + n)])
    xs = Scaler(xalgo); xs.fit(Xr[:N]); ys = Scaler(yalgo); ys.fit(yr[:N])
    D, S, M = 3, 2, 40
    params = synth.make_params(seed, D, S, M, abc=(-1.0, 0.0, -4.0))
    _, alpha, Li = O.forward(np.ascontiguousarray(xs.forward_transform(Xr[:N])), np.ascontiguousarray(ys.forward_transform(yr[:N])), params,
                             S, M, gauss_hermite=False)
    rho = rng.choice(RHO_VALUES, size=(n, 4), p=(0.125, 0.25, 0.375, 0.25))
    return dict(D=D, S=S, M=M, xs=xs, ys=ys, params=params, alpha=alpha, Li=Li, Xr=Xr[N:], yr=yr[N:], dY=dY[N:], rho=rho)


def problem(D, S, M, N0, n, dims=None, seed=0, T=100):
    """The inputs of the parity tiers: parameters; N0 rows with targets for the fit that is updated; n points with their values yn,
    derivatives G (n x nd) along dims and precisions rho; T fresh test rows.  Values and derivatives come from one function of the model
    class, f = phi(x)^T w0, with noise of variance kappa on the values and kappa / rho on a derivative (rho = 0: kappa).  rho is drawn
    from RHO_VALUES with P(0) = 1 / 8; a point whose entries all came out 0 gets 1 in its first."""
    sd = 0x5CF6A000 + 131 * M + seed
    params = synth.make_params(sd + 0x0202, D, S, M, abc=(-1.0, 0.0, -1.0))
    rng = np.random.default_rng(sd)
    K = 2 * (S + M)
    kap = float(np.log1p(np.exp(params[2])))
    w0 = rng.standard_normal(K) / np.sqrt(K)
    X0 = synth.make_X(sd, N0, D); Xn = synth.make_X(sd + 1, n, D); Xs = synth.make_X(sd + 2, T, D)
    f = lambda X: O.feature_map(X, params, D, S, M) @ w0
    y0 = (f(X0) + np.sqrt(kap) * rng.standard_normal(N0))[:, None]
    yn = f(Xn) + np.sqrt(kap) * rng.standard_normal(n)
    dd = list(range(D)) if dims is None else list(dims)
    rho = rng.choice(RHO_VALUES, size=(n, len(dd)), p=(0.125, 0.25, 0.375, 0.25))
    rho[np.all(rho == 0, axis=1), 0] = 1.0
    G = mean_grad(Xn, w0, params, S, M)[:, dd]
    G = G + np.sqrt(kap / np.where(rho > 0, rho, 1.0)) * rng.standard_normal(G.shape)
    return dict(params=params, X0=X0, y0=y0, Xn=Xn, yn=yn, G=G, rho=rho, Xs=Xs, dims=None if dims is None else list(dims), w0=w0)
