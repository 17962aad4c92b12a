"""
numpy restatement of scfgp_acquire_kg (include/scfgp_hip.h; scfgp_amd/csrc/kg.hip), in the device's own forms and order of operations,
and the independent truth it is measured against.

With d_r = u_r - max u <= 0 and b_ir = cov(x_i, x_r) / sigma_i, the knowledge gradient of candidate i is KG_i = E max_r (d_r + b_ir Z).
The device reduces every row of b at the caller's nodes z_1 < ... < z_J (exactly one of them 0.0):

    m_ij = max_r (d_r + b_ir z_j)   (t = b z, then d + t: two roundings)     s_ij = b_ir at the maximiser, ties to the lowest r
    bmin_i, bmax_i = min_r, max_r b_ir

and forms kg <= KG <= kg_hi from the table (bounds()).  kg_exact is the sorted upper-envelope algorithm of Frazier, Powell & Dayanik
over all R lines.
"""
import numpy as np

from tests import acquire_ref as A

argmax = A.argmax
DEFAULT_NODES = np.linspace(-5.0, 5.0, 31)

# (exact - kg) / max exact at DEFAULT_NODES, the largest over tests/test_kg_ref.py's fits (K = 42 and 128, R = 33, 257, 2000, noisy and
# noise-free candidates); that test asserts it within 4 x.
MEASURED_DEFAULT_GAP = 1.4e-2
# the error of bounds() against 50-digit arithmetic on the same node tables (those fits and synthetic lines whose breakpoints reach the
# tails of h), max_i |delta| / max_i kg_hi, the larger of kg's and kg_hi's;
# tests/test_kg_ref.py asserts it within 4 x, the GPU tier bounds the device by 8 x this.
MEASURED_KG_ERR = 1.0e-15


def check_nodes(z):
    """the host-side checks of the entry point"""
    z = np.asarray(z, np.float64).reshape(-1)
    if not 3 <= z.size <= 32:
        raise ValueError('J must lie in 3..32')
    if not np.isfinite(z).all():
        raise FloatingPointError('non-finite nodes')
    if not (np.diff(z) > 0).all():
        raise ValueError('the nodes must be strictly increasing')
    if np.count_nonzero(z == 0.0) != 1:
        raise ValueError('exactly one node must be 0.0')
    return z


def slopes(cov, sd):
    """b (T, R) = cov / sigma_i: cov (T, R) the cross covariance of candidates and reference rows, sd (T,) the candidates' sigma"""
    return np.asarray(cov, np.float64) / np.asarray(sd, np.float64).reshape(-1, 1)


def offsets(mu_ref, minimize=False):
    """d_r = u_r - max u, u = sgn mu"""
    u = (-1.0 if minimize else 1.0) * np.asarray(mu_ref, np.float64).reshape(-1)
    return u - u.max()


def node_table(d, B, z, tie='lowest'):
    """(m (T, J), s (T, J), bmin (T,), bmax (T,)) with the device's two roundings and tie rule (tie='highest': a mutant)"""
    d = np.asarray(d, np.float64).reshape(-1); B = np.asarray(B, np.float64); z = np.asarray(z, np.float64).reshape(-1)
    T, R = B.shape
    m = np.empty((T, z.size)); s = np.empty((T, z.size))
    rows = np.arange(T)
    for j, zj in enumerate(z):
        t = B * zj
        cand = d[None, :] + t
        arg = np.argmax(cand, axis=1) if tie == 'lowest' else R - 1 - np.argmax(cand[:, ::-1], axis=1)
        m[:, j] = cand[rows, arg]; s[:, j] = B[rows, arg]
    return m, s, B.min(axis=1), B.max(axis=1)


def bounds(m, s, bmin, bmax, z, clamp=True):
    """(kg, kg_hi) from the node table, by kg_finish_kernel's recurrence (clamp=False: a mutant without the two clamps)"""
    z = check_nodes(z)
    m = np.asarray(m, np.float64); s = np.asarray(s, np.float64)
    fz = A.h(-np.abs(z))
    T, J = m.shape
    mp, sp = m[:, 0], s[:, 0]
    sk, ik = sp, mp - sp * z[0]
    qp = np.asarray(bmin, np.float64).reshape(-1)
    kg = np.zeros(T); hi = np.zeros(T)
    for j in range(1, J):
        mj, sj = m[:, j], s[:, j]
        zl, zr = z[j - 1], z[j]
        qj = (mj - mp) / (zr - zl)
        if clamp:
            qj = np.minimum(np.maximum(qj, sp), sj)
        hi = hi + np.maximum(qj - qp, 0.0) * fz[j - 1]
        qp = qj
        upd = sj > sk
        ij = mj - sj * zr
        with np.errstate(all='ignore'):
            c = (ik - ij) / (sj - sk)
            if clamp:
                c = np.minimum(np.maximum(c, zl), zr)
            term = (sj - sk) * A.h(-np.abs(c))
        kg = np.where(upd, kg + np.where(upd, term, 0.0), kg)
        sk = np.where(upd, sj, sk); ik = np.where(upd, ij, ik)
        mp, sp = mj, sj
    hi = hi + np.maximum(np.asarray(bmax, np.float64).reshape(-1) - qp, 0.0) * fz[J - 1]
    return kg, hi


def envelope(a, b):
    """the upper envelope of the lines a_r + b_r z (Frazier, Powell & Dayanik 2009, algorithm 1): sort by slope, keep the highest of equal
    slopes, drop the dominated lines.  Returns (slopes of the envelope's lines in rising order, their offsets, the breakpoints between
    consecutive ones)."""
    a = np.asarray(a, np.float64).reshape(-1); b = np.asarray(b, np.float64).reshape(-1)
    order = np.lexsort((a, b))
    a, b = a[order], b[order]
    keep = np.r_[b[1:] != b[:-1], True]                           # the last of a run of equal slopes has the largest offset
    a, b = a[keep], b[keep]
    idx, c = [0], [-np.inf]
    for i in range(1, a.size):
        while True:
            k = idx[-1]
            ck = (a[k] - a[i]) / (b[i] - b[k])
            if ck <= c[-1]:
                idx.pop(); c.pop()
                continue
            idx.append(i); c.append(ck)
            break
    return b[idx], a[idx], np.array(c[1:])


def kg_exact(a, b):
    """E max_r (a_r + b_r Z) - max_r a_r = sum_k (b_{k+1} - b_k) f(-|c_k|) over the breakpoints c_k of the envelope of ALL lines: the
    independent truth"""
    bb, _, c = envelope(a, b)
    return float(np.sum(np.diff(bb) * A.h(-np.abs(c)))) if c.size else 0.0


def kg_exact_rows(d, B):
    return np.array([kg_exact(d, row) for row in np.asarray(B, np.float64)])
