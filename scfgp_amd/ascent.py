"""
Batched, deterministic projected-gradient ascent in a box: the host side of continuous Thompson sampling / max-value entropy search
(SCFGP.sample_maximize).  Every row is an independent problem (its own function, named by sidx) that shares each evaluation call with
the others, so one iteration of all rows costs one call of `fg` per backtracking trial -- with fg = HipEngine.sample_grad, one device
call for all samples.
"""
import numpy as np

ARMIJO = 1e-4          # sufficient-increase constant of the line search
MAX_HALVINGS = 30      # trials per iteration before a row is given up (its step has shrunk by 2^-30)


def _pg_norm(X, g, lo, hi):
    """norm of the ascent direction g with the components that push out of the box at an active bound removed"""
    g = np.where((X <= lo) & (g < 0), 0.0, g)
    g = np.where((X >= hi) & (g > 0), 0.0, g)
    return np.sqrt((g * g).sum(1))


def ascend(fg, X0, sidx, lo, hi, minimize=False, max_iter=60, gtol=1e-6):
    """Maximise (minimize: minimise) row by row over the box [lo, hi].

    fg(X, sidx) -> (val (n,), grad (n, D)) evaluates row i of X under function sidx[i]; X0 (T, D) are the starts, inside the box; lo, hi
    are scalars or (D,).  Each iteration takes, per row, the step X <- clip(X + t g) with the row's own step size t: a Barzilai-Borwein
    value s.s / |s.y| from the second iteration on (s, y: the last change of the point and of the gradient), halved until Armijo's
    condition f(X+) >= f(X) + 1e-4 g.(X+ - X) holds.  Every trial is ONE call of fg on the rows that still need it.  A row whose step
    fails 30 halvings keeps its point and leaves the iteration unconverged; a row stops as converged when its projected-gradient norm is
    <= gtol max(1, |val|).

    Returns (X (T, D), val (T,), converged (T,) bool, n_calls).  By construction a row's value never decreases (minimize: never
    increases) relative to fg's value at X0, and X stays in the box."""
    X = np.array(X0, dtype=np.float64, ndmin=2)
    T, D = X.shape
    sidx = np.asarray(sidx).reshape(-1)
    if sidx.size != T:
        raise ValueError('ascend: sidx has %d entries for %d rows' % (sidx.size, T))
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float64), (D,))
    hi = np.broadcast_to(np.asarray(hi, dtype=np.float64), (D,))
    if (lo > hi).any():
        raise ValueError('ascend: lo exceeds hi')
    if ((X < lo) | (X > hi)).any():
        raise ValueError('ascend: a start lies outside the box')
    sign = -1.0 if minimize else 1.0

    def call(rows, Xr):
        v, g = fg(Xr, sidx[rows])
        return sign * np.asarray(v, dtype=np.float64).reshape(-1), sign * np.asarray(g, dtype=np.float64).reshape(len(rows), D)

    everyone = np.arange(T)
    val, grad = call(everyone, X)
    n_calls = 1
    diag = float(np.sqrt(((hi - lo) ** 2).sum()))
    gn = np.sqrt((grad * grad).sum(1))
    # first step: a tenth of the box's diagonal along the gradient
    step = np.where(gn > 0, 0.1 * (diag if diag > 0 else 1.0) / np.where(gn > 0, gn, 1.0), 1.0)
    converged = np.zeros(T, dtype=bool)
    stalled = np.zeros(T, dtype=bool)
    for _ in range(int(max_iter)):
        converged |= _pg_norm(X, grad, lo, hi) <= gtol * np.maximum(1.0, np.abs(val))
        pending = np.flatnonzero(~converged & ~stalled)
        if pending.size == 0:
            break
        t = step.copy()
        for _trial in range(MAX_HALVINGS):
            Xt = np.clip(X[pending] + t[pending, None] * grad[pending], lo, hi)
            d = Xt - X[pending]
            vt, gt = call(pending, Xt)
            n_calls += 1
            gd = np.maximum((grad[pending] * d).sum(1), 0.0)
            ok = vt >= val[pending] + ARMIJO * gd                  # NaN compares false: a non-finite trial is a failed one
            acc = pending[ok]
            if acc.size:
                s, y = d[ok], gt[ok] - grad[acc]
                ss, sy = (s * s).sum(1), np.abs((s * y).sum(1))
                bb = np.where((sy > 0) & (ss > 0), ss / np.where(sy > 0, sy, 1.0), 2.0 * t[acc])
                step[acc] = np.clip(bb, 1e-12, 1e12)
                X[acc], val[acc], grad[acc] = Xt[ok], vt[ok], gt[ok]
            pending = pending[~ok]
            if pending.size == 0:
                break
            t[pending] *= 0.5
        stalled[pending] = True
    converged |= _pg_norm(X, grad, lo, hi) <= gtol * np.maximum(1.0, np.abs(val))
    return X, sign * val, converged, n_calls
