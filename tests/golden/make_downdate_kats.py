"""
Regenerates tests/golden/downdate_kats.npz: near-singular cases of scfgp_loo, scfgp_forget and scfgp_condition (tests/downdate_range.py
has the case table and the error models) with 60-digit mpmath truths.  Needs mpmath, here only; a few minutes on eight cores.

Per shape  data/<D>_<S>_<M>/X, y            the rows and targets every fit of that shape takes a prefix of
Per fit    fit/<fit>/params, alpha, Li      the INPUTS as doubles: alpha and the lower triangle of Li as the oracle's forward gave them here.
                                            The truths below are the exact functions of THESE doubles (LAPACK and libm differ between
                                            machines, so the inputs are stored, not regenerated)
loo/<fit>_b<block>/   mu, std (N), joint, gap = 1 - lam_max (per block), den_mu, den_std (N), den_joint (per block): the models of
                      tests/downdate_range.py, margin: the admission figure min gap / (u (K + b) || |C||C|^T + I ||)
lev/<fit>/            lev, den_lev (N): the leverages and their model, the same for every block size
forget/<fit>_keep<k>/ alpha, Li (lower), A (lower; A' = L S L^T with L = Li^-1: into tests/golden/downdate_resid_kats.npz), joint, pivot2 = min M_ii^2, lam_min (of S)
cond/<fit>_add<n>/    alpha, Li (lower), A (as above), lam_min, lam_max (of S)
pivot/<fit>_row<i>_x<k>/  alpha, pivot2, joint, lam_min of the PIVOT_CASES (k copies of a row; the last pivot is the smallest: asserted)
boundary/             rows, copies, h (2 each): the (row, k) of BOUNDARY_FIT, k in BOUNDARY_COPIES, whose k h is nearest to 1 from below and
                      from above (k copies of a row of leverage h: S = I - k c c^T, lam_min = 1 - k h); alpha, pivot2, joint, lam_min: the truths
                      of scfgp_forget on the first
ref/<case>/<kind>     the numpy restatement's constant here;  cref/<kind>: its maximum over the admitted cases (C_REF)
The feature map is evaluated in mpmath from X and the parameters (column means over axis 0, s = e^b sqrt(2 / M)).
"""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', '..'))
from oracle import scfgp_oracle as O        # noqa: E402
from tests import downdate_range as R       # noqa: E402

DPS = 60


def _mp():
    import mpmath
    mpmath.mp.dps = DPS
    return mpmath.mp


def to_mp(a):
    mp = _mp()
    a = np.asarray(a, np.float64)
    return [mp.mpf(float(v)) for v in a] if a.ndim == 1 else [[mp.mpf(float(v)) for v in row] for row in a]


def to_f64(a):
    return np.array([[float(v) for v in row] for row in a]) if a and isinstance(a[0], list) else np.array([float(v) for v in a])


def mp_features(X, params, D, S, M):
    """Phi (n rows of K = 2 (S + M)) as oracle.feature_map defines it, in mpmath from the doubles X and params"""
    mp = _mp()
    p = to_mp(params)
    b = p[1]
    t = 3
    l_F = [p[t + d * S:t + (d + 1) * S] for d in range(D)]; t += D * S
    r_F = [p[t + m * S:t + (m + 1) * S] for m in range(M)]; t += M * S
    l_P = p[t:t + S]; t += S
    P = p[t:t + M]
    F = [[mp.fdot(l_F[d], r_F[m]) for m in range(M)] for d in range(D)]
    cols = [[l_F[d][s] for d in range(D)] for s in range(S)] + [[F[d][m] for d in range(D)] for m in range(M)]
    off = [l_P[s] - mp.fsum(cols[s]) / D for s in range(S)] + [P[m] - mp.fsum(cols[S + m]) / D for m in range(M)]
    s = mp.exp(b) * mp.sqrt(mp.mpf(2) / M)
    out = []
    for x in to_mp(X):
        z = [mp.fdot(x, cols[j]) + off[j] for j in range(S + M)]
        out.append([s * mp.cos(v) for v in z] + [s * mp.sin(v) for v in z])
    return out


def mp_chol(A):
    mp = _mp()
    n = len(A)
    L = [[mp.mpf(0)] * n for _ in range(n)]
    for i in range(n):
        for j in range(i):
            L[i][j] = (A[i][j] - mp.fdot(L[i][:j], L[j][:j])) / L[j][j]
        d = A[i][i] - mp.fdot(L[i][:i], L[i][:i])
        assert d > 0, 'not positive definite in mpmath'
        L[i][i] = mp.sqrt(d)
    return L


def mp_fwd(L, b):
    """L^-1 b for a vector b"""
    mp = _mp()
    x = []
    for i in range(len(L)):
        x.append((b[i] - mp.fdot(L[i][:i], x)) / L[i][i])
    return x


def mp_bwd(L, b):
    """L^-T b"""
    mp = _mp()
    n = len(L)
    x = [mp.mpf(0)] * n
    for i in range(n - 1, -1, -1):
        x[i] = (b[i] - mp.fsum(L[k][i] * x[k] for k in range(i + 1, n))) / L[i][i]
    return x


def mp_lam_min(A, L):
    """smallest eigenvalue of the symmetric positive definite A = L L^T: float64's eigenvector, three inverse iterations, Rayleigh quotient"""
    mp = _mp()
    n = len(A)
    v = to_mp(np.linalg.eigh(to_f64(A))[1][:, 0])
    for _ in range(3):
        v = mp_bwd(L, mp_fwd(L, v))
        nv = mp.sqrt(mp.fdot(v, v))
        v = [x / nv for x in v]
    return mp.fdot(v, [mp.fdot(A[i], v) for i in range(n)])


def mp_C(Phi, Li):
    mp = _mp()
    K = len(Li)
    return [[mp.fdot(row[:j + 1], Li[j][:j + 1]) for j in range(K)] for row in Phi]


def mp_update(C, r, alpha, Li, sign, kap, with_A=False):
    """the K x K stage of forget (sign -1) / condition (+1) in mpmath"""
    mp = _mp()
    K = len(Li); n = len(C)
    Ct = [[C[i][j] for i in range(n)] for j in range(K)]
    Sm = [[None] * K for _ in range(K)]
    for i in range(K):
        for j in range(i + 1):
            Sm[i][j] = Sm[j][i] = (1 if i == j else 0) + sign * mp.fdot(Ct[i], Ct[j])
    Mc = mp_chol(Sm)
    Lit = [[Li[i][j] for i in range(K)] for j in range(K)]                      # columns of Li
    cols = [[mp.mpf(0)] * j + mp_fwd([row[j:] for row in Mc[j:]], Lit[j][j:]) for j in range(K)]
    Li_new = [[cols[j][i] for j in range(K)] for i in range(K)]
    w = mp_fwd(Mc, [mp.fdot(Ct[j], r) for j in range(K)])
    gamma = mp_bwd(Mc, w)
    alpha_new = [alpha[j] + sign * mp.fdot(Lit[j], gamma) for j in range(K)]
    joint = -(((mp.fdot(r, r) + mp.fdot(w, w)) / kap + n * mp.log(2 * mp.pi * kap) - 2 * mp.fsum(mp.log(Mc[i][i]) for i in range(K))) / 2)
    lam = mp_lam_min(Sm, Mc)
    A = None
    if with_A:                                                   # A' = L S L^T, L = Li^-1
        ident = [[mp.mpf(1 if i == j else 0) for i in range(K)] for j in range(K)]
        Lc = [mp_fwd(Li, ident[j]) for j in range(K)]           # Lc[j]: column j of L
        Lr = [[Lc[j][i] for j in range(K)] for i in range(K)]   # rows of L
        LS = [[mp.fdot(Lr[i], Sm[j]) for j in range(K)] for i in range(K)]
        A = R.pack(to_f64([[mp.fdot(LS[i], Lr[j]) if j <= i else mp.mpf(0) for j in range(K)] for i in range(K)]))
    return dict(alpha=to_f64(alpha_new), Li=R.pack(to_f64(Li_new)), joint=float(joint), pivot2=float(min(Mc[i][i] for i in range(K)) ** 2),
                argmin=int(np.argmin([float(Mc[i][i]) for i in range(K)])), A=A, lam=float(lam), lam_max=float(np.linalg.eigvalsh(to_f64(Sm))[-1]))


def mp_loo(Phi, C, y, alpha, kap, block, Li64, alpha64):
    """every block's truths and models"""
    mp = _mp()
    n = len(C); K = len(C[0])
    out = dict((k, []) for k in ('mu', 'std', 'lev', 'joint', 'gap', 'den_mu', 'den_std', 'den_lev', 'den_joint'))
    norm = 0.0
    for i0 in range(0, n, block):
        i1 = min(n, i0 + block); b = i1 - i0
        Cb = C[i0:i1]
        H = [[mp.fdot(Cb[i], Cb[j]) for j in range(b)] for i in range(b)]
        IH = [[(1 if i == j else 0) - H[i][j] for j in range(b)] for i in range(b)]
        r = [y[i0 + i] - mp.fdot(Phi[i0 + i], alpha) for i in range(b)]
        Rc = mp_chol(IH)
        W = [mp_fwd(Rc, [mp.mpf(1 if k == j else 0) for k in range(b)]) for j in range(b)]     # W[j]: column j of R^-1
        t = mp_fwd(Rc, r)
        e = mp_bwd(Rc, t)
        mu = [y[i0 + i] - e[i] for i in range(b)]
        sd = [mp.sqrt(kap * mp.fdot(W[j], W[j])) for j in range(b)]
        gap = IH[0][0] if b == 1 else mp_lam_min(IH, Rc)
        G = [[mp.fdot(W[i], W[j]) for j in range(b)] for i in range(b)]
        joint = -((mp.fdot(t, t) / kap + b * mp.log(2 * mp.pi * kap) - 2 * mp.fsum(mp.log(Rc[i][i]) for i in range(b))) / 2)
        Phi64 = to_f64(Phi[i0:i1]); C64 = to_f64(Cb)
        dens, dj = R.loo_models(Phi64, C64, np.abs(Phi64) @ np.abs(Li64).T, alpha64, to_f64(y[i0:i1]), to_f64(G), to_f64(sd), to_f64(e),
                                float(mp.fdot(t, t)), float(gap), float(kap), K)
        norm = max(norm, float(np.linalg.norm(np.abs(C64) @ np.abs(C64).T + np.eye(b), 2)))
        for k, v in dens.items():
            out[k].append(v)
        out['mu'].append(to_f64(mu)); out['std'].append(to_f64(sd)); out['lev'].append(np.array([float(H[i][i]) for i in range(b)]))
        out['joint'].append([float(joint)]); out['gap'].append([float(gap)]); out['den_joint'].append([dj])
    out = dict((k, np.concatenate(v)) for k, v in out.items())
    out['margin'] = float(out['gap'].min() / (R.U64 * (K + block) * norm))
    return out


def fit_task(fit):
    """everything that starts from one fit"""
    mp = _mp()
    fx = R.Fixture(INPUTS)
    D, S, M, N, params, X, y, alpha64, Li64 = fx.fit(fit)
    ncond = max([n for f, n in R.COND_CASES if f == fit] + [0])
    Xall, yall = fx.rows(fit, 0, N + ncond)
    Phi = mp_features(Xall, params, D, S, M)
    Li = to_mp(Li64); alpha = to_mp(alpha64.ravel()); ym = to_mp(yall)
    C = mp_C(Phi, Li)
    kap = mp.log1p(mp.exp(mp.mpf(float(params[2]))))
    res = [mp.mpf(ym[i]) - mp.fdot(Phi[i], alpha) for i in range(len(Phi))]
    out = {}
    for f, blocks in R.LOO_CASES:
        if f == fit:
            for block in blocks:
                o = mp_loo(Phi[:N], C[:N], ym[:N], alpha, kap, block, Li64, alpha64)
                out['lev/%s/lev' % fit] = o.pop('lev'); out['lev/%s/den_lev' % fit] = o.pop('den_lev')        # the same for every block
                out.update(('%s/%s' % (R.lkey(fit, block), k), v) for k, v in o.items())
                print('%-28s min gap %.2e margin %.2e' % (R.lkey(fit, block), o['gap'].min(), o['margin']), flush=True)
    for f, keep in R.FORGET_CASES:
        if f == fit:
            o = mp_update(C[keep:N], res[keep:N], alpha, Li, -1, kap, with_A=True)
            o['lam_min'] = o.pop('lam'); del o['lam_max'], o['argmin']
            out.update(('%s/%s' % (R.fkey(fit, keep), k), v) for k, v in o.items())
            print('%-28s lam_min %.2e pivot2 %.2e' % (R.fkey(fit, keep), o['lam_min'], o['pivot2']), flush=True)
    for f, n in R.COND_CASES:
        if f == fit:
            o = mp_update(C[N:N + n], res[N:N + n], alpha, Li, 1, kap, with_A=True)
            o['lam_min'] = o.pop('lam'); del o['pivot2'], o['joint'], o['argmin']
            out.update(('%s/%s' % (R.ckey(fit, n), k), v) for k, v in o.items())
            print('%-28s lam_max %.2e lam_min %.2e' % (R.ckey(fit, n), o['lam_max'], o['lam_min']), flush=True)
    for f, row, k in R.PIVOT_CASES:
        if f == fit:
            o = mp_update([C[row]] * k, [res[row]] * k, alpha, Li, -1, kap)
            assert o['argmin'] == len(Li) - 1, 'the last pivot is not the smallest'
            out.update(('%s/%s' % (R.pkey(fit, row, k), kk), o[kk2]) for kk, kk2 in (('alpha', 'alpha'), ('pivot2', 'pivot2'), ('joint', 'joint'),
                                                                                      ('lam_min', 'lam')))
            print('%-28s lam_min %.2e pivot2 %.2e (the last pivot)' % (R.pkey(fit, row, k), o['lam'], o['pivot2']), flush=True)
    if fit == R.BOUNDARY_FIT:
        h = out['lev/%s/lev' % fit]
        kh = np.array([k * h for k in R.BOUNDARY_COPIES])                  # (copies, rows)
        lo = np.where(kh < 1.0, kh, -np.inf); hi = np.where(kh > 1.0, kh, np.inf)
        picks = [np.unravel_index(np.argmax(lo), kh.shape), np.unravel_index(np.argmin(hi), kh.shape)]
        rows = np.array([p[1] for p in picks]); ks = np.array([R.BOUNDARY_COPIES[p[0]] for p in picks])
        assert ks[0] * h[rows[0]] < 1.0 < ks[1] * h[rows[1]]
        i, k = int(rows[0]), int(ks[0])
        o = mp_update([C[i]] * k, [res[i]] * k, alpha, Li, -1, kap)
        out.update({'boundary/rows': rows, 'boundary/copies': ks, 'boundary/h': h[rows], 'boundary/alpha': o['alpha'], 'boundary/pivot2': o['pivot2'],
                    'boundary/joint': o['joint'], 'boundary/lam_min': o['lam']})
        print('boundary rows %s copies %s h %s, the first: lam_min %.3e pivot2 %.3e' % (rows, ks, h[rows], o['lam'], o['pivot2']), flush=True)
    return out


INPUTS = {}


def main():
    INPUTS.update(R.make_inputs())
    for fit, (D, S, M, N, a, b) in R.FITS.items():
        X = INPUTS[R.shape_key(D, S, M) + '/X'][:N]; y = INPUTS[R.shape_key(D, S, M) + '/y'][:N]
        _, alpha, Li = O.forward(np.ascontiguousarray(X), y.reshape(-1, 1), INPUTS['fit/%s/params' % fit], S, M, gauss_hermite=False)
        INPUTS['fit/%s/alpha' % fit] = np.asarray(alpha).ravel(); INPUTS['fit/%s/Li' % fit] = R.pack(np.tril(Li))
    out = dict(INPUTS)
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:       # forked: the children see INPUTS
        for o in pool.imap_unordered(fit_task, sorted(R.FITS, key=lambda f: -R.FITS[f][3] * (R.FITS[f][1] + R.FITS[f][2]) ** 2)):
            out.update(o)
    fx = R.Fixture(out)
    # coverage conditions
    gaps = []
    for fit, blocks in R.LOO_CASES:
        for block in blocks:
            if fx.admitted(fit, block):
                gaps.append(float(out[R.lkey(fit, block) + '/gap'].min()))
    dropped = [R.lkey(f, b) for f, bs in R.LOO_CASES for b in bs if not fx.admitted(f, b)]
    print('loo cases dropped by the admission rule:', dropped)
    assert min(gaps) <= 1e-7, min(gaps)
    assert min(float(out[R.fkey(f, k) + '/lam_min']) for f, k in R.FORGET_CASES) <= 1e-10
    # the numpy restatement's own constants and C_REF
    ratios = R.all_ratios(fx)
    for key, r in R.cond32_reference(fx).items():
        ratios[key].update(r)
    for key, r in ratios.items():
        for kind, v in r.items():
            out['ref/%s/%s' % (key, kind)] = v
        print('%-28s %s' % (key, ' '.join('%s=%.3g' % kv for kv in r.items())))
    w = R.worst(ratios)
    for kind in R.KINDS + R.PRINTED:
        out['cref/' + kind] = w[kind][0]
    print('C_REF', R.fmt(w))
    path = os.path.join(HERE, 'downdate_kats.npz')
    np.savez_compressed(path, **dict((k, v) for k, v in out.items() if not k.endswith('/A')))
    print('%s: %d bytes' % (path, os.path.getsize(path)))
    np.savez_compressed(R.RESID_FIXTURE, **dict((k, v) for k, v in out.items() if k.endswith('/A')))
    print('%s: %d bytes' % (R.RESID_FIXTURE, os.path.getsize(R.RESID_FIXTURE)))


if __name__ == '__main__':
    main()
