"""
numpy fp64 form of the greedy choice by integrated variance reduction (include/scfgp_hip.h: scfgp_select_iv).  With C = Phi_c Li^T of
the pool, C_R = Phi_r Li^T of the reference rows with weights omega, Q = C_R^T diag(omega) C_R, d_i = |c_i|^2 and a_i = c_i^T Q c_i,
step j does

    p_j = argmax over the rows not yet taken with w_i > 0 of w_i a_i / (1 + d_i)        (ties: the lowest index)
    t = c_p - sum_{l<j} u_l (u_l . c_p),  dp = c_p . t,  u_j = t / sqrt(1 + dp)
    h = Q u_j,  q = u_j . h,  g = h - sum_{l<j} u_l (u_l . h),  v = g - (q / 2) u_j
    s = C u_j,  z = C v,  a <- max(a - 2 s z, 0),  d <- max(d - s^2, 0)

`replay` runs the same downdates along a GIVEN pick sequence and returns a, d and the scores before every step, so another
implementation's picks can be judged one by one.  `half_q` = False drops the (q / 2) u_j term: the mutation the CPU tier must catch.
"""
import numpy as np

from tests.select_ref import _direction


def gram(CR, omega=None):
    """Q = C_R^T diag(omega) C_R"""
    CR = np.asarray(CR, np.float64)
    return CR.T @ CR if omega is None else CR.T @ (np.asarray(omega, np.float64).ravel()[:, None] * CR)


def subset_reference(T):
    """the issue's second reference set: rows pool[::3] with weights 0.5 + default_rng(1).random(R)"""
    rows = np.arange(0, T, 3)
    return rows, 0.5 + np.random.default_rng(1).random(len(rows))


def _scores(w, a, d, taken):
    return np.where((w > 0) & ~taken, w * a / (1.0 + d), -np.inf)


def _step(C, Q, U, p, a, d, half_q=True):
    u, dp = _direction(C, U, p)
    h = Q @ u
    q = float(u @ h)
    g = h - U.T @ (U @ h) if len(U) else h.copy()
    v = g - (0.5 * q) * u if half_q else g
    s = C @ u; z = C @ v
    return u, dp, q, np.maximum(a - 2.0 * s * z, 0.0), np.maximum(d - s * s, 0.0)


def select(C, Q, m, w=None, kap=1.0, half_q=True):
    """dict(idx (m,), red (m,) = kap q_j, var (m,) = kap dp_j, ivar (2,) = kap tr Q and that minus the reductions, a, d (T,): after the
    m picks, a0, d0: the start values, std_after (T,), gap (m,): relative gap between the best and the second-best score at every step
    (inf where one eligible row is left), U (m, K))"""
    C = np.asarray(C, np.float64); Q = np.asarray(Q, np.float64)
    T, K = C.shape
    w = np.ones(T) if w is None else np.asarray(w, np.float64).ravel()
    d = np.sum(C * C, axis=1)
    a = np.einsum('ik,ik->i', C @ Q, C)
    a0, d0 = a.copy(), d.copy()
    taken = np.zeros(T, bool)
    U = np.empty((0, K))
    idx, red, var, gap = [], [], [], []
    iv0 = kap * float(np.trace(Q)); iv = iv0
    for j in range(m):
        s = _scores(w, a, d, taken)
        p = int(np.argmax(s))                                   # the first of equal maxima
        assert np.isfinite(s[p]), 'fewer than m eligible rows'
        rest = np.delete(s, p)
        second = rest.max() if rest.size else -np.inf
        gap.append((s[p] - second) / s[p] if np.isfinite(second) and s[p] > 0 else np.inf)
        u, dp, q, a, d = _step(C, Q, U, p, a, d, half_q)
        U = np.vstack([U, u])
        taken[p] = True
        idx.append(p); red.append(kap * q); var.append(kap * dp)
        iv = iv - kap * q
    return dict(idx=np.array(idx, np.int64), red=np.array(red), var=np.array(var), ivar=np.array([iv0, iv]), a=a, d=d, a0=a0, d0=d0,
                std_after=np.sqrt(kap * (1.0 + d)), gap=np.array(gap), U=U)


def replay(C, Q, w, idx):
    """(m + 1, T) a and d: row j is the state before pick j of the GIVEN sequence idx, row m after all of them; the (m, T) scores of the
    rows that were eligible at step j (-inf elsewhere); and q (m,): the reduction of every pick in units of kappa"""
    C = np.asarray(C, np.float64); Q = np.asarray(Q, np.float64)
    T, K = C.shape
    w = np.ones(T) if w is None else np.asarray(w, np.float64).ravel()
    d = np.sum(C * C, axis=1)
    a = np.einsum('ik,ik->i', C @ Q, C)
    taken = np.zeros(T, bool)
    U = np.empty((0, K))
    As, Ds, scores, qs = [a.copy()], [d.copy()], [], []
    for p in np.asarray(idx).ravel():
        p = int(p)
        scores.append(_scores(w, a, d, taken))
        u, dp, q, a, d = _step(C, Q, U, p, a, d)
        U = np.vstack([U, u])
        taken[p] = True
        As.append(a.copy()); Ds.append(d.copy()); qs.append(q)
    return np.array(As), np.array(Ds), np.array(scores), np.array(qs)


def scale(ref, kap):
    """kappa max_i a_i / (1 + d_i) of the start values: the size the recurrence of red and ivar rounds at"""
    return kap * float((ref['a0'] / (1.0 + ref['d0'])).max())
