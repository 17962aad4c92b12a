"""
numpy restatement of the greedy Monte-Carlo batch expected improvement (include/scfgp_hip.h: scfgp_select_qei) on a given block

    F (T, nsamp): the sample functions at the pool rows (sample_ref.samples, or the library's own scfgp_sample output)
    sgn = +1, or -1 when minimising;  u = sgn F;  b = sgn best + xi;  row t is eligible iff w is None or w[t] > 0
    start   m_s = b, or max(b, max_r sgn P[r][s]) with the pending rows' values P (np, nsamp)
    step j  score_t = (1 / nsamp) sum_s max(u_ts - m_s, 0) for every row
            p_j = the lowest eligible, not yet taken t at which score_t is largest (sample_argmax_ref's rule)
            gain[j] = score_{p_j};  m_s <- max(m_s, u_{p_j, s})
    qei = [(1 / nsamp) sum_s (m_s - b) at the start, the same after the last pick]

A term that is not > 0 (a NaN among them) counts as 0, as on the device.  The two keyword switches of `greedy` are the mutations that
tests/test_select_qei_ref.py must catch.
"""
import itertools

import numpy as np


def scores(u, m):
    """score_t of every row of u (T, nsamp) against m (nsamp,)"""
    d = u - m[None, :]
    with np.errstate(invalid='ignore'):
        return np.where(d > 0.0, d, 0.0).sum(axis=1) / float(u.shape[1])


def start(nsamp, best, xi=0.0, minimize=False, pending=None):
    """(b, m at the start)"""
    sgn = -1.0 if minimize else 1.0
    b = sgn * float(best) + float(xi)
    m = np.full(nsamp, b)
    if pending is not None and np.size(pending):
        m = np.maximum(m, (sgn * np.asarray(pending, np.float64).reshape(-1, nsamp)).max(axis=0))
    return b, m


def qei_of(m, b):
    return float(np.sum(m - b)) / float(m.size)


def greedy(F, m_picks, best, xi=0.0, w=None, pending=None, minimize=False, forget_taken=False, update_before_gain=False):
    """(idx (m,) int64, gain (m,), score0 (T,), mstate (nsamp,), qei (2,))"""
    F = np.asarray(F, np.float64)
    T, nsamp = F.shape
    u = -F if minimize else F
    free = np.ones(T, bool) if w is None else np.asarray(w, np.float64) > 0
    if m_picks < 1 or m_picks > np.count_nonzero(free):
        raise ValueError('m = %d but only %d rows are eligible' % (m_picks, np.count_nonzero(free)))
    free = free.copy()
    b, m = start(nsamp, best, xi, minimize, pending)
    qei = [qei_of(m, b), 0.0]
    idx = np.empty(m_picks, np.int64); gain = np.empty(m_picks)
    score0 = None
    for j in range(m_picks):
        sc = scores(u, m)
        if j == 0:
            score0 = sc
        rows = np.flatnonzero(free)
        p = int(rows[np.argmax(sc[rows])])                        # numpy: the first occurrence, i.e. the lowest row
        if update_before_gain:
            m = np.maximum(m, u[p])
            sc = scores(u, m)
        idx[j] = p; gain[j] = sc[p]
        if not forget_taken:
            free[p] = False
        m = np.maximum(m, u[p])
    qei[1] = qei_of(m, b)
    return idx, gain, score0, m, np.array(qei)


def top_two_gaps(F, m_picks, best, xi=0.0, w=None, pending=None, minimize=False):
    """at every pick of `greedy`, (top - runner_up) / top of the eligible untaken scores (inf where the runner-up does not exist;
    nan where the top score is 0)"""
    F = np.asarray(F, np.float64)
    u = -F if minimize else F
    free = (np.ones(F.shape[0], bool) if w is None else np.asarray(w, np.float64) > 0).copy()
    _, m = start(F.shape[1], best, xi, minimize, pending)
    out = []
    for _ in range(m_picks):
        sc = scores(u, m)
        rows = np.flatnonzero(free)
        order = rows[np.argsort(-sc[rows], kind='stable')]
        top = sc[order[0]]
        with np.errstate(all='ignore'):
            out.append(np.inf if order.size < 2 else (top - sc[order[1]]) / top)
        free[order[0]] = False
        m = np.maximum(m, u[order[0]])
    return np.array(out)


def batch_qei(F, rows, best, xi=0.0, minimize=False, pending=None):
    """the Monte-Carlo q-EI of the batch `rows` (plus the pending rows), from the definition"""
    F = np.asarray(F, np.float64)
    u = -F if minimize else F
    b, m = start(F.shape[1], best, xi, minimize, pending)
    return qei_of(np.maximum(m, u[list(rows)].max(axis=0)), b)


def exhaustive(F, m_picks, best, xi=0.0, minimize=False):
    """the best q-EI over all batches of m_picks rows"""
    return max(batch_qei(F, rows, best, xi, minimize) for rows in itertools.combinations(range(np.shape(F)[0]), m_picks))
