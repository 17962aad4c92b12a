"""
numpy fp64 form of the greedy maximum-information choice (include/scfgp_hip.h: scfgp_select): with C = Phi_c Li^T of the pool
(tests/pred_cov_ref.py: factor), d_i = |c_i|^2 and weights w, step j does

    p_j = argmax over the rows not yet taken with w_i > 0 of w_i d_i        (ties: the lowest index)
    t = c_p - sum_{l<j} u_l (u_l . c_p),  dp = c_p . t,  u_j = t / sqrt(1 + dp)
    d_i <- max(d_i - (c_i . u_j)^2, 0)

`replay` runs the same downdates along a GIVEN pick sequence and returns d before every step, so another implementation's picks can be
judged one by one.
"""
import numpy as np

from tests import pred_cov_ref

# the issue's table: (D, S, M, N0, T, m); fits on the first N0 rows of loo_ref.problem(D, S, M, N0 + T, ABC), the pool is the next T rows
ABC = (-1.0, 0.0, -1.0)
CASES = [(5, 4, 60, 1000, 1000, 40), (3, 1, 20, 150, 150, 150), (20, 20, 280, 3000, 700, 64), (64, 32, 1024, 1500, 600, 24)]
LONG = (5, 4, 60, 1000, 32768 + 300, 8)         # two chunks; w = 0 on all but 50 rows that straddle row 32768
LONG3 = (5, 4, 60, 1000, 65536 + 300, 8)        # three chunks (a buffer of the row feed is reused); 50 such rows at each of 32768 and 65536


def kappa(params):
    return pred_cov_ref.kappa(params)


def long_weights(T=LONG[4]):
    w = np.zeros(T)
    for b in range(32768, T, 32768):
        w[b - 25:b + 25] = 1.0
    return w


def _direction(C, U, p):
    cp = C[p]
    t = cp - U.T @ (U @ cp) if len(U) else cp.copy()
    dp = float(cp @ t)
    return t / np.sqrt(1.0 + dp), dp


def _scores(w, d, taken):
    s = np.where((w > 0) & ~taken, w * d, -np.inf)
    return s


def select(C, m, w=None, kap=1.0):
    """dict(idx (m,), var (m,) = kap dp_j, gain (m,) = log1p(dp_j) / 2, d (T,): d after the m picks, std_after (T,), gap (m,): relative gap
    between the best and the second-best score at every step (inf where one eligible row is left))"""
    C = np.asarray(C, np.float64)
    T, K = C.shape
    w = np.ones(T) if w is None else np.asarray(w, np.float64).ravel()
    d = np.sum(C * C, axis=1)
    taken = np.zeros(T, bool)
    U = np.empty((0, K))
    idx, var, gain, gap = [], [], [], []
    for j in range(m):
        s = _scores(w, d, taken)
        p = int(np.argmax(s))                                   # the first of equal maxima
        assert np.isfinite(s[p]), 'fewer than m eligible rows'
        rest = np.delete(s, p)
        second = rest.max() if rest.size else -np.inf
        gap.append((s[p] - second) / s[p] if np.isfinite(second) and s[p] > 0 else np.inf)
        u, dp = _direction(C, U, p)
        U = np.vstack([U, u])
        d = np.maximum(d - (C @ u) ** 2, 0.0)
        taken[p] = True
        idx.append(p); var.append(kap * dp); gain.append(0.5 * np.log1p(dp))
    return dict(idx=np.array(idx, np.int64), var=np.array(var), gain=np.array(gain), d=d, std_after=np.sqrt(kap * (1.0 + d)),
                gap=np.array(gap))


def replay(C, w, idx):
    """(m + 1, T): row j is d before pick j of the GIVEN sequence idx, row m is d after all of them; and the (m, T) scores w_i d_i of
    the rows that were eligible at step j (-inf elsewhere)"""
    C = np.asarray(C, np.float64)
    T, K = C.shape
    w = np.ones(T) if w is None else np.asarray(w, np.float64).ravel()
    d = np.sum(C * C, axis=1)
    taken = np.zeros(T, bool)
    U = np.empty((0, K))
    ds, scores = [d.copy()], []
    for p in np.asarray(idx).ravel():
        p = int(p)
        scores.append(_scores(w, d, taken))
        u, _ = _direction(C, U, p)
        U = np.vstack([U, u])
        d = np.maximum(d - (C @ u) ** 2, 0.0)
        taken[p] = True
        ds.append(d.copy())
    return np.array(ds), np.array(scores)


def problem(case):
    """(params, X0, y0, Xpool) of a row of CASES / LONG / LONG3"""
    from tests import loo_ref
    D, S, M, N0, T, m = case
    params, X, y = loo_ref.problem(D, S, M, N0 + T, ABC)
    return params, np.ascontiguousarray(X[:N0]), np.ascontiguousarray(y[:N0]), np.ascontiguousarray(X[N0:])
