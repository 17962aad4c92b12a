"""
numpy fp64 form of the exact leave-block-out predictions (include/scfgp_hip.h: scfgp_loo): with a fit A = Phi^T Phi + lam I = L L^T,
Li = L^-1, alpha = A^-1 Phi^T y on ALL rows and a block I of b of its rows, with the oracle's features Phi_I,

    C = Phi_I Li^T,  H = C C^T,  r = y_I - Phi_I alpha,  I - H = R R^T,  e = (I - H)^-1 r,  mu^{-I} = y_I - e,
    sigma_i = sqrt(kappa [(I - H)^-1]_ii),  log p(y_I | rest) = -1/2 [ |R^-1 r|^2 / kappa + b log(2 pi kappa) - 2 sum log R_ii ]

(Woodbury on A - Phi_I^T Phi_I), and `refit`: the same numbers the slow way, one oracle fit per block on the other rows.
"""
import numpy as np

from oracle import scfgp_oracle as O

# the issue's table: (D, S, M, N, block), (a, b, c) of the hyper-parameters
CASES = [((5, 4, 60, 400, 1), (-1.0, 0.0, -1.0)), ((5, 4, 60, 400, 7), (-1.0, 0.0, -1.0)), ((5, 4, 60, 400, 64), (-1.0, 0.0, -1.0)),
         ((3, 1, 20, 150, 1), (-1.0, 0.0, -1.0)), ((20, 20, 280, 640, 16), (-1.0, 0.0, -1.0)), ((5, 4, 60, 150, 8), (-1.0, 0.0, -1.0)),
         ((5, 4, 60, 400, 1), (-3.0, 0.0, -1.0))]


def kappa(params):
    return float(np.log1p(np.exp(params[2])))


def blocks(n, block):
    return [(i, min(n, i + block)) for i in range(0, n, block)]


def problem(D, S, M, N, abc=(-1.0, 0.0, -1.0)):
    """tests/condition_ref.problem's rows and targets, parameters with the given (a, b, c)"""
    from scfgp_amd import synth
    from tests import condition_ref
    _, X, y, _ = condition_ref.problem(D, S, M, N, 0)
    params = synth.make_params(0x5CF67000 + M + 0x0202, D, S, M, abc=abc)
    return params, X, y


def loo(X, y, alpha, Li, params, S, M, block=1):
    """dict(mu (n,), std (n,), lev (n,), e (n,), joint (nblocks,), lmax (nblocks,): largest eigenvalue of each H_I, stats (8,)) from
    scaled rows X (n,D) and scaled targets y that are in the fit (alpha, Li); entries of Li above the diagonal are not read"""
    X = np.asarray(X, np.float64); y = np.asarray(y, np.float64).ravel()
    n = X.shape[0]
    Li = np.tril(np.asarray(Li, np.float64)); alpha = np.asarray(alpha, np.float64).reshape(-1, 1)
    kap = kappa(params)
    mu = np.empty(n); sd = np.empty(n); lev = np.empty(n); joint = []; lmax = []
    for i0, i1 in blocks(n, block):
        Phi = O.feature_map(X[i0:i1], params, X.shape[1], S, M)
        C = Phi @ Li.T
        H = C @ C.T
        r = y[i0:i1] - (Phi @ alpha).ravel()
        R = np.linalg.cholesky(np.eye(i1 - i0) - H)
        W = np.linalg.inv(R)
        t = W @ r
        mu[i0:i1] = y[i0:i1] - W.T @ t
        sd[i0:i1] = np.sqrt(kap * np.sum(W * W, axis=0))
        lev[i0:i1] = np.diag(H)
        joint.append(-0.5 * (t @ t / kap + (i1 - i0) * np.log(2 * np.pi * kap) - 2.0 * np.sum(np.log(np.diag(R)))))
        lmax.append(float(np.linalg.eigvalsh(H)[-1]))
    e = y - mu
    marg = -0.5 * (e ** 2 / sd ** 2 + np.log(2 * np.pi * sd ** 2))
    joint = np.array(joint)
    stats = np.array([n, np.sum(e ** 2), np.sum(np.abs(e)), np.sum(marg), np.sum(joint), lev.max(), len(joint), 0.0])
    return dict(mu=mu, std=sd, lev=lev, e=e, marg=marg, joint=joint, lmax=np.array(lmax), stats=stats)


def row_lmax(ref, n, block):
    """lmax of every row's own block (n,)"""
    return np.repeat(ref['lmax'], block)[:n]


def refit(X, y, params, S, M, block=1, with_joint=False):
    """(mu (n,), std (n,)) of every row from the oracle's fit on all rows but those of its block and the oracle's predict; with_joint:
    also the log density of y_I under that fit's joint Gaussian N(mu_I, kappa (I + Phi_I A_-I^-1 Phi_I^T)) per block"""
    X = np.asarray(X, np.float64); y = np.asarray(y, np.float64).reshape(-1, 1)
    n = X.shape[0]
    kap = kappa(params)
    mu = np.empty(n); sd = np.empty(n); joint = []
    for i0, i1 in blocks(n, block):
        keep = np.r_[0:i0, i1:n]
        _, a, L = O.forward(np.ascontiguousarray(X[keep]), np.ascontiguousarray(y[keep]), params, S, M, gauss_hermite=False)
        m, s = O.predict(np.ascontiguousarray(X[i0:i1]), a, L, params, S, M)
        mu[i0:i1] = np.asarray(m).ravel(); sd[i0:i1] = np.asarray(s).ravel()
        if with_joint:
            C = O.feature_map(X[i0:i1], params, X.shape[1], S, M) @ np.tril(L).T
            cov = kap * (np.eye(i1 - i0) + C @ C.T)
            d = y[i0:i1].ravel() - mu[i0:i1]
            _, logdet = np.linalg.slogdet(cov)
            joint.append(-0.5 * (d @ np.linalg.solve(cov, d) + logdet + (i1 - i0) * np.log(2 * np.pi)))
    return (mu, sd, np.array(joint)) if with_joint else (mu, sd)
