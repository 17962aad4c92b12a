"""
numpy fp64 form of the greedy maximum-information choice (include/scfgp_hip.h: scfgp_select): with C = Phi_c Li^T of the pool
(tests/pred_cov_ref.py: factor), d_i = |c_i|^2 and weights w, step j does

    p_j = argmax over the rows not yet taken with w_i > 0 of w_i d_i        (ties: the lowest index)
    t = c_p - sum_{l<j} u_l (u_l . c_p),  dp = c_p . t,  u_j = t / sqrt(1 + dp)
    d_i <- max(d_i - (c_i . u_j)^2, 0)

`replay` runs the same downdates along a GIVEN pick sequence and returns d before every step, so another implementation's picks can be
judged one by one; `replay_chol` returns the same from one Cholesky factorisation of the picked rows' Gram matrix (BLAS-3: for
thousands of picks).  `synthetic_problem` is the input of the shapes at the documented bounds of K and m, where no fit is affordable.
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


def rows_per_group(T):
    """select.hip's select_rows_per_group: rows per workgroup of the sweeps, 64 doubled until there are at most 4096 groups"""
    rpw = 64
    while (T + rpw - 1) // rpw > 4096:
        rpw *= 2
    return rpw


def edge_rows(T):
    """about 64 rows at the places where the index arithmetic of the sweeps can go wrong: row 0 and row T - 1, the first and the last
    row of several groups of rows_per_group(T) rows (the last, possibly ragged, group among them), the rows on both sides of three
    32768-row chunk boundaries, and rows in between"""
    rpw = rows_per_group(T)
    ng = (T + rpw - 1) // rpw
    rows = {0, T - 1}
    for g in (0, 1, 7, ng // 3, ng // 2, ng - 3, ng - 2, ng - 1):
        rows |= {g * rpw, min((g + 1) * rpw, T) - 1}
    rows |= {min((ng - 1) * rpw + 1, T - 1), T - 2}              # two more of the last group (or its neighbour)
    nb = (T - 1) // 32768
    for b in (1, nb // 2, nb):
        rows |= {b * 32768 - 1, b * 32768}
    rng = np.random.default_rng(T)
    rows |= set(rng.integers(0, T, 64 - len(rows)).tolist())
    return np.array(sorted(rows), np.int64)


def edge_weights(T):
    """w > 0 on edge_rows(T) only: unequal weights in [1, 2), row T - 1 the heaviest (10) and its neighbour T - 2 next (6): tuned on the
    reference, whose picks under both criteria then take the two rows in the middle of the sequence (d varies 15-fold over the rows)"""
    rows = edge_rows(T)
    w = np.zeros(T)
    w[rows] = 1.0 + np.random.default_rng(T + 1).random(len(rows))
    w[T - 2] = 6.0
    w[T - 1] = 10.0
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


def replay_chol(C, w, idx):
    """`replay` without the loop over the picks, for sequences too long for it: with C_P the picked rows in order,
    L = chol(I + C_P C_P^T) and V = L^-1 C_P C^T (m, T), d before step j is d0 - sum_{l<j} V[l]^2 and dp_j = L_jj^2 - 1 (row j of
    L^-1 C_P is u_j: the Cholesky factor orthogonalises the picks in order, as the recurrence does).  Returns `replay`'s two arrays
    and dp (m,).  No clamp at 0: d is a difference of exact sums here, not a recurrence."""
    from scipy.linalg import solve_triangular
    C = np.asarray(C, np.float64)
    T = C.shape[0]
    idx = np.asarray(idx, np.int64).ravel()
    m = len(idx)
    w = np.ones(T) if w is None else np.asarray(w, np.float64).ravel()
    CP = C[idx]
    L = np.linalg.cholesky(np.eye(m) + CP @ CP.T)
    V = solve_triangular(L, CP @ C.T, lower=True, check_finite=False)
    ds = np.empty((m + 1, T))
    ds[0] = np.sum(C * C, axis=1)
    np.cumsum(V * V, axis=0, out=ds[1:])
    ds[1:] = ds[0] - ds[1:]
    free = np.ones((m, T), bool)
    free[:, w <= 0] = False
    for j in range(1, m):
        free[j:, idx[j - 1]] = False
    scores = np.where(free, w * ds[:m], -np.inf)
    return ds, scores, np.diag(L) ** 2 - 1.0


def synthetic_factor(K, seed=0):
    """a dense, well-conditioned lower-triangular Li for shapes at which no fit is affordable (the selection entry points read only Li
    and the parameters): diagonal 1 + U(0, 1), strict lower part N(0, (0.5 / sqrt(K))^2)"""
    rng = np.random.default_rng(seed)
    Li = np.tril(rng.standard_normal((K, K)), -1)
    Li *= 0.5 / np.sqrt(K)
    Li[np.diag_indices(K)] = 1.0 + rng.random(K)
    return Li


def synthetic_problem(D, S, M, T, seed=0):
    """(params with (a, b, c) = ABC, Li = synthetic_factor(K), pool rows (T, D))"""
    from oracle import scfgp_oracle as O
    from scfgp_amd import synth
    rng = np.random.default_rng(seed + 1)
    params = O.init_params(D, S, M, rng)
    params[:3] = ABC
    return params, synthetic_factor(2 * (S + M), seed), synth.make_X(0x5E1EC7 + seed, T, D)


def problem(case):
    """(params, X0, y0, Xpool) of a row of CASES / LONG / LONG3"""
    from tests import loo_ref
    D, S, M, N0, T, m = case
    params, X, y = loo_ref.problem(D, S, M, N0 + T, ABC)
    return params, np.ascontiguousarray(X[:N0]), np.ascontiguousarray(y[:N0]), np.ascontiguousarray(X[N0:])
