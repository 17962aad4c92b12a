"""
Restatements of the O(P) kernels either side of the sweeps (scfgp_amd/csrc/kernels_params.hip), not a test: a helper of
tests/test_hyper_ref.py, tests/test_gpu_hyper_range.py and tests/golden/make_hyper_kats.py.

  numpy float64, in the device's operation order
    scalars          scal_kernel: s, e2a, lam, kappa, em2a, sigc from a, b, c
    pen_rows         pen_rows_kernel: row means and population stds of F (over M) and l_F (over S); 256-thread strided partials,
                     then the halving tree
    pen_sums         pen_sums_kernel: the four sums over d in order, and R_PEN
    fbar, lbar       fbar_kernel and lbar_kernel: the centring and penalty terms of Fbar and lbar_F, dense and rank-S form
    finalize         finalize_kernel: cost and grad[0:3] from the stage scalars
  `mutate` swaps in one wrong formula (the mutation checks of the CPU tier): 'kappa_plain' log(1 + e^c), 'lam_e2a' no jitter,
  'sample_std' n - 1, 'no_mean_term' the penalty gradient without 2 mu / n.

  mpmath, 60 digits
    mp_scalars, mp_penalty, mp_penalty_grad (central differences of mp_penalty), and mp_objective / mp_grad: the whole objective at a
    tiny shape -- feature map, A = Phi^T Phi + (e^{2a} + 1e-6) I, its Cholesky, alpha, Li, the closed-form expectation term
    (oracle.forward, gauss_hermite=False), penalty, cost, predictive mu* and std* -- and its gradient by central differences with a
    step of 1e-25: a plain reference that shares nothing with the analytic gradient of the library or of the oracle.
"""
import numpy as np

EPSILON = 1e-6              # the jitter in lam (SCFGP.py:93,105)
DPS = 60                    # mpmath working digits
FD_STEP = '1e-25'           # central differences at 60 digits: truncation ~ h^2 = 1e-50, rounding ~ 1e-60 / h = 1e-35

# Worst relative error of the CORRECT numpy restatement against mpmath over the grids of tests/test_hyper_ref.py (a in [-8, 3],
# b in [-6, 6] at M = 5 and 300, c in [-36, 36]; measured with numpy 's libm on x86-64).  The CPU tier allows 2 x these, the GPU tier
# 4 x (the device's exp / log1p are other implementations, an ulp or two apart, and the GPU tier reads kappa through sqrt and a square)
MEASURED_SCALAR_ERR = {
    's': 2.4e-16,           # exp, sqrt, a division and a product
    'e2a': 9.7e-17,
    'lam': 1.5e-16,
    'kappa': 2.1e-16,       # c > 0: c + log1p(e^-c); else log1p(e^c)
    'em2a': 9.7e-17,
    'sigc': 1.6e-16,
}
# Worst error of the correct restatement on the penalty edge rows (tests/test_hyper_ref.py), against mpmath: row means over
# max |row|, row stds and R_PEN relative, the penalty gradient over max |gradient| of its matrix
MEASURED_PEN_ERR = {
    'mean': 1.6e-16,
    'std': 1.5e-16,         # two passes: the mean's rounding shifts every deviation alike, second order in the sum of squares
    'pen': 2.5e-16,
    'grad': 6.1e-13,        # (x - mean) / std at |mean| / std = 5e3..1e4: the mean's rounding, |mean| u, is 1e4 u of the deviation
}


# the grids of the CPU tier; the GPU tier walks B_GRID and C_GRID through the public API
A_GRID = np.linspace(-8.0, 3.0, 89)            # step 1 / 8: holds -7, -6, -4, 2
B_GRID = np.linspace(-6.0, 6.0, 97)            # step 1 / 8: holds -4, 4
C_GRID = np.linspace(-36.0, 36.0, 289)         # step 1 / 4: holds -30, -20, -14, -10, 10, 30
C_FAR = (-700.0, -100.0, 100.0, 700.0)         # finiteness, monotonicity and the asymptotes only
M_GRID = (5, 300)
PEN_SHAPES = [(3, 2, 5), (3, 2, 300), (3, 70, 5), (2, 70, 300)]      # (D, S, M): either side of the 256-thread and 64-lane strides


# ---- numpy, device order ---------------------------------------------------------------------------------------------------------
def softplus(c):
    """kappa as scal_kernel forms it"""
    c = np.float64(c)
    return c + np.log1p(np.exp(-c)) if c > 0 else np.log1p(np.exp(c))


def scalars(a, b, c, M, mutate=None):
    a, b, c = np.float64(a), np.float64(b), np.float64(c)
    with np.errstate(over='ignore', under='ignore'):
        s = np.exp(b) * np.sqrt(2.0 / M)
        e2a = np.exp(2.0 * a)
        lam = e2a if mutate == 'lam_e2a' else e2a + EPSILON
        kappa = np.log(1.0 + np.exp(c)) if mutate == 'kappa_plain' else softplus(c)
        em2a = np.exp(-2.0 * a)
        sigc = 1.0 / (1.0 + np.exp(-c))
    return dict(s=s, e2a=e2a, lam=lam, kappa=kappa, em2a=em2a, sigc=sigc)


def strided_tree_sum(x, width):
    """thread t adds x[t], x[t + width], .. in order; then red[t] += red[t + m] for m = width / 2 .. 1 (the shared-memory tree of
    pen_rows_kernel, width 256; lane 0 of lbar_kernel's xor butterfly, width 64)"""
    x = np.asarray(x, np.float64)
    part = np.zeros(width)
    for k0 in range(0, x.size, width):
        seg = x[k0:k0 + width]
        part[:seg.size] += seg
    m = width // 2
    while m >= 1:
        part[:m] += part[m:2 * m]
        m //= 2
    return part[0]


def pen_rows(l_F, F, mutate=None):
    """(mF, sF, ml, sl): per-row mean and population std of F over M and of l_F over S"""
    out = []
    with np.errstate(invalid='ignore', divide='ignore'):
        for T in (np.asarray(F, np.float64), np.asarray(l_F, np.float64)):
            n = T.shape[1]
            mean = np.array([strided_tree_sum(r, 256) / n for r in T])
            dev = T - mean[:, None]
            ss = np.array([strided_tree_sum(r * r, 256) for r in dev])
            out += [mean, np.sqrt(ss / (n - 1 if mutate == 'sample_std' else n))]
    return tuple(out)


def pen_sums(stats, S, M):
    """(mu_w, sig_w, mu_l, sig_l) and R_PEN; kl(mu, sig) = sig + mu^2 - log sig, weights M and S"""
    s = []
    for q in stats:
        t = 0.0
        for v in q:
            t += v
        s.append(np.float64(t))
    mu_w, sig_w, mu_l, sig_l = s
    with np.errstate(divide='ignore', invalid='ignore'):
        pen = ((sig_w + mu_w * mu_w - np.log(sig_w)) * M + (sig_l + mu_l * mu_l - np.log(sig_l)) * S) / (S + M)
    return (mu_w, sig_w, mu_l, sig_l), pen


def penalty(l_F, F, mutate=None):
    l_F = np.asarray(l_F, np.float64); F = np.asarray(F, np.float64)
    return pen_sums(pen_rows(l_F, F, mutate), l_F.shape[1], F.shape[1])[1]


def _pen_term(T, mean, std, mu, sig, wgt, mutate):
    n = T.shape[1]
    with np.errstate(invalid='ignore', divide='ignore'):
        t = (1.0 - 1.0 / sig) * (T - mean[:, None]) / (n * std[:, None])
        return wgt * (t if mutate == 'no_mean_term' else t + 2.0 * mu / n)


def pen_grad(l_F, F, mutate=None):
    """(d R_PEN / d F, d R_PEN / d l_F): the penalty terms of fbar_kernel and lbar_kernel"""
    l_F = np.asarray(l_F, np.float64); F = np.asarray(F, np.float64)
    S, M = l_F.shape[1], F.shape[1]
    mF, sF, ml, sl = pen_rows(l_F, F, mutate)
    (mu_w, sig_w, mu_l, sig_l), _ = pen_sums((mF, sF, ml, sl), S, M)
    return (_pen_term(F, mF, sF, mu_w, sig_w, float(M) / (S + M), mutate),
            _pen_term(l_F, ml, sl, mu_l, sig_l, float(S) / (S + M), mutate))


def fbar(l_F, F, XZ=None, TZ=None, mutate=None):
    """fbar_kernel.  Dense form: XZ ((D + 1) x J) = X~^T Zbar, row D the column sums: Fbar = XZ[d][S + m] - XZ[D][S + m] / D + penalty.
    Rank-S form: TZ ((S + 1) x J) = T~^T Zbar, row S the column sums: the data term stays factored, Fbar = -TZ[S][S + m] / D + penalty"""
    D, S = np.shape(l_F)
    pen = pen_grad(l_F, F, mutate)[0]
    if TZ is not None:
        return -np.asarray(TZ)[S, S:][None, :] / D + pen
    XZ = np.asarray(XZ)
    return XZ[:D, S:] - XZ[D, S:][None, :] / D + pen


def lbar(l_F, r_F, F, Fb, XZ=None, TZ=None, XU=None, mutate=None):
    """lbar_kernel before its 1 / N: sum_m Fbar[d][m] r_F[m][s] on 64 strided lanes, + the direct term - column sum / D + penalty;
    rank-S form: XU (D x S) = X^T (Zbar_L + Zbar_M r_F) holds the direct term and the data part of Fbar r_F"""
    l_F = np.asarray(l_F, np.float64); r_F = np.asarray(r_F, np.float64)
    D, S = l_F.shape
    pen = pen_grad(l_F, F, mutate)[1]
    out = np.empty((D, S))
    for d in range(D):
        for s in range(S):
            v = strided_tree_sum(Fb[d] * r_F[:, s], 64)
            if TZ is not None:
                v += (XU[d][s] - TZ[S][s] / D) + pen[d, s]
            else:
                v += (XZ[d][s] - XZ[D][s] / D) + pen[d, s]
            out[d, s] = v
    return out


def finalize(sc, a, st, M, N):
    """finalize_kernel: st holds T1 (log det), T2, kbar, sumqv, sumpmu (t2kb[0..3]), yy, gtalpha, trabar, trag, utg, pen"""
    T3 = sc['em2a'] * (st['yy'] - st['gtalpha'])
    T4 = 2.0 * (N - M) * a
    cost = (st['T1'] + st['T2'] + T3 + T4 + st['pen']) / N
    ga = (2.0 * sc['e2a'] * st['trabar'] - 2.0 * T3 + 2.0 * (N - M)) / N
    bbar = 2.0 * st['trag'] + st['utg'] + 2.0 * st['sumqv'] + st['sumpmu']
    return cost, np.array([ga, bbar / N, st['kbar'] * sc['sigc'] / N])


# ---- penalty edge rows -----------------------------------------------------------------------------------------------------------
EDGE_CASES = ('lF_offset', 'F_offset', 'sig_small', 'sig_large')


def edge_factors(name, D, S, M, seed=0x5CF6B000):
    """(l_F (D, S), r_F (M, S)) whose rows sit on an edge of the penalty statistics; F = l_F r_F^T
      lF_offset   a row of l_F = 5 + 1e-3 noise: |mean| / std >= 1e3
      F_offset    the rows of r_F agree to 1e-4: every row of F is a constant + 1e-4 noise, |mean| / std >= 1e3
      sig_small   l_F x 0.01: the sums of the stds of l_F and of F are well below 1 (log sig < 0, 1 - 1 / sig < 0)
      sig_large   l_F x 3 + distinct row offsets: both sums well above 1"""
    from scfgp_amd import synth
    seed = seed + 1000 * S + M
    l_F = synth.normal(seed, 0, D * S).reshape(D, S); r_F = synth.uniform(seed + 2, 0, M * S).reshape(M, S)
    noise = synth.normal(seed + 4, 0, M * S).reshape(M, S)
    if name == 'lF_offset':
        l_F[0] = 5.0 + 1e-3 * noise.ravel()[:S]
    elif name == 'F_offset':
        r_F = r_F[:1] + 1e-4 * noise
    elif name == 'sig_small':
        l_F *= 0.01
    elif name == 'sig_large':
        l_F = 3.0 * l_F + np.arange(D)[:, None]
    else:
        raise KeyError(name)
    return l_F, r_F


def edge_params(name, D, S, M, abc=(-1.0, 0.0, -1.0)):
    """the flat parameter vector of an edge case (phases uniform in [0, 2 pi))"""
    from scfgp_amd import synth
    l_F, r_F = edge_factors(name, D, S, M)
    return np.concatenate((np.asarray(abc, np.float64), l_F.ravel(), r_F.ravel(), 2 * np.pi * synth.uniform(0x5CF6B777, 0, S + M)))


# ---- mpmath ----------------------------------------------------------------------------------------------------------------------
def _mp():
    import mpmath
    mpmath.mp.dps = DPS
    return mpmath.mp


def mp_scalars(a, b, c, M):
    mp = _mp()
    a, b, c = mp.mpf(float(a)), mp.mpf(float(b)), mp.mpf(float(c))
    e2a = mp.exp(2 * a)
    return dict(s=mp.exp(b) * mp.sqrt(mp.mpf(2) / M), e2a=e2a, lam=e2a + mp.mpf(EPSILON), kappa=mp.log1p(mp.exp(c)),
                em2a=mp.exp(-2 * a), sigc=1 / (1 + mp.exp(-c)))


def _mp_rows(T):
    mp = _mp()
    return [[x if isinstance(x, mp.mpf) else mp.mpf(float(x)) for x in row] for row in T]


def _mp_stats(T):
    mp = _mp()
    n = len(T[0])
    means = [mp.fsum(r) / n for r in T]
    stds = [mp.sqrt(mp.fsum([(x - m) ** 2 for x in r]) / n) for r, m in zip(T, means)]
    return means, stds


def mp_penalty(l_F, F):
    """(R_PEN, (mF, sF, ml, sl)) in mpmath; l_F, F: rows of floats or mpf"""
    mp = _mp()
    l_F, F = _mp_rows(l_F), _mp_rows(F)
    S, M = len(l_F[0]), len(F[0])
    mF, sF = _mp_stats(F); ml, sl = _mp_stats(l_F)
    kl = lambda mu, sig: sig + mu ** 2 - mp.log(sig)
    pen = (kl(mp.fsum(mF), mp.fsum(sF)) * M + kl(mp.fsum(ml), mp.fsum(sl)) * S) / (S + M)
    return pen, (mF, sF, ml, sl)


def sample_columns(n):
    """columns of a row of length n at which the penalty gradient is checked: all of a short row; of a long one both ends and either
    side of the 64-lane and 256-thread strides"""
    return list(range(n)) if n <= 8 else sorted(set(k for k in (0, 1, 31, 63, 64, 65, 255, 256, 257, n - 2, n - 1) if k < n))


def mp_penalty_grad(l_F, F):
    """(d R_PEN / d F, d R_PEN / d l_F) with F and l_F as independent variables, by central differences, at sample_columns() of every
    row: two dicts (d, k) -> value"""
    mp = _mp()
    h = mp.mpf(FD_STEP)
    l_F, F = _mp_rows(l_F), _mp_rows(F)
    out = []
    for which in (1, 0):
        T = (l_F, F)[which]
        g = {}
        for d in range(len(T)):
            for k in sample_columns(len(T[0])):
                x = T[d][k]
                T[d][k] = x + h; up = mp_penalty(l_F, F)[0]
                T[d][k] = x - h; dn = mp_penalty(l_F, F)[0]
                T[d][k] = x
                g[(d, k)] = (up - dn) / (2 * h)
        out.append(g)
    return out[0], out[1]


class MpProblem(object):
    """the whole objective in mpmath on fixed data: X (N, D), y (N,), test rows Xs (T, D), all float64 and taken exactly"""

    def __init__(self, X, y, S, M, Xs=None):
        mp = _mp()
        self.X = _mp_rows(np.asarray(X, np.float64)); self.y = [mp.mpf(float(v)) for v in np.asarray(y, np.float64).ravel()]
        self.Xs = None if Xs is None else _mp_rows(np.asarray(Xs, np.float64))
        self.N, self.D, self.S, self.M = len(self.X), len(self.X[0]), S, M
        self.J = S + M; self.K = 2 * self.J
        self.P = 3 + self.D * S + M * S + S + M

    def params(self, p):
        mp = _mp()
        return [v if isinstance(v, mp.mpf) else mp.mpf(float(v)) for v in p]

    def _unpack(self, p):
        mp = _mp()
        D, S, M = self.D, self.S, self.M
        l_F = [p[3 + d * S:3 + (d + 1) * S] for d in range(D)]
        o = 3 + D * S
        r_F = [p[o + m * S:o + (m + 1) * S] for m in range(M)]
        o += M * S
        ph = p[o:o + S + M]
        F = [[mp.fdot(l_F[d], r_F[m]) for m in range(M)] for d in range(D)]
        W = [l_F[d] + F[d] for d in range(D)]
        cols = [[W[d][j] for d in range(D)] for j in range(self.J)]
        off = [ph[j] - mp.fsum(cols[j]) / D for j in range(self.J)]
        return l_F, F, cols, off

    def _phi(self, rows, cols, off, s):
        mp = _mp()
        out = []
        for x in rows:
            cs = [mp.cos_sin(mp.fdot(x, cols[j]) + off[j]) for j in range(self.J)]
            out.append([s * c for c, _ in cs] + [s * t for _, t in cs])
        return out

    def evaluate(self, p, full=False):
        """cost; full: dict(cost, alpha, Li, A, pen, mu, std)"""
        mp = _mp()
        p = self.params(p)
        N, M, K = self.N, self.M, self.K
        a, b, c = p[0], p[1], p[2]
        l_F, F, cols, off = self._unpack(p)
        s = mp.exp(b) * mp.sqrt(mp.mpf(2) / M)
        lam = mp.exp(2 * a) + mp.mpf(EPSILON)
        kappa = mp.log1p(mp.exp(c))
        Phi = self._phi(self.X, cols, off, s)
        PhiT = [[Phi[n][k] for n in range(N)] for k in range(K)]
        A = [[None] * K for _ in range(K)]
        for i in range(K):
            for j in range(i + 1):
                A[i][j] = A[j][i] = mp.fdot(PhiT[i], PhiT[j])
            A[i][i] += lam
        g = [mp.fdot(PhiT[k], self.y) for k in range(K)]
        yy = mp.fdot(self.y, self.y)
        L = [[mp.mpf(0)] * K for _ in range(K)]
        for j in range(K):
            L[j][j] = mp.sqrt(A[j][j] - mp.fdot(L[j][:j], L[j][:j]))
            for i in range(j + 1, K):
                L[i][j] = (A[i][j] - mp.fdot(L[i][:j], L[j][:j])) / L[j][j]
        Li = [[mp.mpf(0)] * K for _ in range(K)]
        for j in range(K):
            Li[j][j] = 1 / L[j][j]
            for i in range(j + 1, K):
                Li[i][j] = -mp.fdot(L[i][j:i], [Li[k][j] for k in range(j, i)]) / L[i][i]
        beta = [mp.fdot(Li[i][:i + 1], g[:i + 1]) for i in range(K)]
        alpha = [mp.fdot([Li[i][k] for i in range(k, K)], beta[k:]) for k in range(K)]
        T1 = 2 * mp.fsum([mp.log(L[j][j]) for j in range(K)])
        two_pi = 2 * mp.pi
        T2 = mp.mpf(0)
        for n in range(N):
            ph = Phi[n]
            v = mp.fsum([mp.fdot(Li[i][:i + 1], ph[:i + 1]) ** 2 for i in range(K)])
            r = mp.fdot(ph, alpha) - self.y[n]
            d = kappa * (v + 1)
            T2 += (r * r + v) / d + mp.log(two_pi * d)
        T3 = mp.exp(-2 * a) * (yy - mp.fdot(g, alpha))
        T4 = 2 * (N - M) * a
        pen = mp_penalty(l_F, F)[0]
        cost = (T1 + T2 + T3 + T4 + pen) / N
        if not full:
            return cost
        out = dict(cost=cost, alpha=alpha, Li=Li, A=A, pen=pen, g=g, yy=yy, T1=T1, T2=T2, T3=T3, T4=T4, Phi=Phi)
        if self.Xs is not None:
            Ps = self._phi(self.Xs, cols, off, s)
            out['mu'] = [mp.fdot(ph, alpha) for ph in Ps]
            out['std'] = [mp.sqrt(kappa * (1 + mp.fsum([mp.fdot(Li[i][:i + 1], ph[:i + 1]) ** 2 for i in range(K)]))) for ph in Ps]
        return out

    def grad_entry(self, p, i):
        """d cost / d p[i] by a central difference"""
        mp = _mp()
        h = mp.mpf(FD_STEP)
        p = self.params(p)
        up = list(p); up[i] = p[i] + h
        dn = list(p); dn[i] = p[i] - h
        return (self.evaluate(up) - self.evaluate(dn)) / (2 * h)


def mp_cond(A):
    """2-norm condition number of the symmetric positive definite A (rows of mpf)"""
    mp = _mp()
    ev = mp.eigsy(mp.matrix(A), eigvals_only=True)
    ev = [ev[i] for i in range(len(ev))]
    return max(ev) / min(ev)


def to_f64(x):
    """float64 rounding of an mpf or of nested rows of them"""
    if isinstance(x, (list, tuple)):
        return np.array([to_f64(v) for v in x], dtype=np.float64)
    return float(x)
