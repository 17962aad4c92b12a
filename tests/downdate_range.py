"""
Near-singular range tests of scfgp_loo, scfgp_forget and scfgp_condition (not a test: the case table, the error models, the ratios and
the mutants shared by tests/golden/make_downdate_kats.py, tests/test_downdate_range_ref.py and tests/test_gpu_downdate_range.py).

The three entry points end in a small factorisation whose conditioning the caller controls: I - H_I per block (loo), S = I -+ C^T C
(forget / condition).  The fixture tests/golden/downdate_kats.npz holds, per case, the INPUTS as doubles (rows, targets, parameters and
the alpha, Li the oracle's forward gave) and the 60-digit mpmath value of the entry point's formulas on exactly those doubles.  An
output is judged by `error / (u * model)`, a constant that stays of order one over nine decades of conditioning:

  forget     model 1 / lam_min(S) for  |D Li'_t|_F / |Li'|_F  per 64-row tile t,  |D alpha'| / |alpha'|,  |D min M_ii^2| / min M_ii^2,
             and  |D joint| / n  (absolute, per removed row)
  condition  model K for the first two (kinds cond_Li, cond_alpha) and, as a second pair of kinds (cond_Li_c, cond_alpha_c), model
             cond(S) = lam_max / lam_min: measured here, u K leaves the restatement's constants between 0.05 and 1e6 (they go with the
             rounding of C^T C against the unit eigenvalues of S), cond(S) between 6e-7 and 1.4; each pair is tight where the other is not
  loo        mu / std per row: max(|D mu|, |D sigma|) against sigma / (1 - lam_max of the row's block), the fp32 bound of
             tests/test_gpu_loo.py with u for eps32 (kind loo_musd);  leverage: 2 sum_j |c_ij| (|Phi||Li|^T)_ij + h_i;  joint (summed
             over the call's blocks): sum_j (|t_j|^2 / kappa + b_j) / (1 - lam_max_j), t = R^-1 r, b_j the block's rows
  The component-wise first-order loo model
                 mu     |G| ((K + b)(|C||C|^T + I) |e| + (K + 2)(|Phi||alpha| + |y|)),        G = (I - H)^-1
                 std    sigma_i / (2 G_ii)  (K + b) (|G| (|C||C|^T + I) |G|)_ii
  is evaluated too (loo_cw_mu, loo_cw_std: printed, not asserted).  Over the 20 admitted fp64 cases and blocks the numpy restatement's
  worst constant per case spreads over 0.64 .. 236 (a factor 370) under the simple model and over 0.00077 .. 3.7 (a factor 4800, the
  larger of mu and std) under the component-wise one, so the simple model is the one asserted; tests/test_downdate_range_ref.py
  prints both spreads.

C_REF[kind] is the largest constant of the numpy restatements (tests/loo_ref.py, forget_ref.py, condition_ref.py) over the admitted
cases, measured by the generator against mpmath and stored in the fixture -- never taken from the device.  The CPU tier holds the
restatements to 4 C_REF on any machine, the GPU tier holds the device to 8 C_REF.

The residual max |Li' A' Li'^T - I| (kinds forget_resid, cond_resid, cond_resid_c; same models) uses A' = L S L^T, L = Li^-1, formed in
mpmath and stored rounded in a second file, tests/golden/downdate_resid_kats.npz.  It sees what the tile-wise norm of D Li' cannot: that
norm is relative to |Li'|_F, which the rows along the near-singular directions dominate, so an error of 1e-4 in a well-scaled row passes
it at lam_min = 9e-9 (mutant li_small_row).  An fp32 context's scfgp_condition (C and C^T C in fp32) is judged in units of eps32 cond(S)
against the restatement with fp32 products (kinds cond32_*).

Sizes: the cases take 48 468 doubles of input triangles (Li of 15 fits) and 46 388 each of Li' and A' truths (ten forget and four
condition cases: 7 x 2080 + 2 x 8256 + 820, 3 x 2080 + 8256), 8 bytes each and incompressible: 388 KB + 371 KB + 371 KB before anything
else, against the 400 KB the case table was budgeted with.  The files are 1.0 MB and 0.37 MB.
"""
import os

import numpy as np

from oracle import scfgp_oracle as O

U64 = 2.0 ** -53
U32 = 2.0 ** -24
TILE = 64
REF_FACTOR = 4.0            # restatement on another machine against C_REF (the acquire-range tier's)
DEV_FACTOR = 8.0            # device against C_REF (the project's margin for device against restatement)
ADMIT = 1e4                 # (1 - lam_max) / (u (K + b) || |C||C|^T + I ||_2) of an admitted loo case
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'downdate_kats.npz')
RESID_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'downdate_resid_kats.npz')     # the A' triangles
SEED = 0x5CF67000

# fits: name -> (D, S, M, N, a, b); c = -1 everywhere.  Rows and targets are the first N of tests/condition_ref.problem's.
FITS = {
    'k64_n256_a1': (8, 8, 24, 256, -1.0, 0.0), 'k64_n256_a4': (8, 8, 24, 256, -4.0, 0.0), 'k64_n256_a7': (8, 8, 24, 256, -7.0, 0.0),
    'k64_n256_a7b3': (8, 8, 24, 256, -7.0, 3.0), 'k64_n62_a4': (8, 8, 24, 62, -4.0, 0.0), 'k64_n62_a7': (8, 8, 24, 62, -7.0, 0.0),
    'k64_n62_a7b3': (8, 8, 24, 62, -7.0, 3.0), 'k64_n32_a7b3': (8, 8, 24, 32, -7.0, 3.0),
    'k128_n64_a7': (5, 4, 60, 64, -7.0, 0.0), 'k128_n136_a7': (5, 4, 60, 136, -7.0, 0.0), 'k40_n160_a7b3': (5, 4, 16, 160, -7.0, 3.0),
    # the fits that scfgp_condition starts from: the first N0 rows
    'k64_n1_a7b3': (8, 8, 24, 1, -7.0, 3.0), 'k64_n16_a7b3': (8, 8, 24, 16, -7.0, 3.0), 'k128_n4_a7': (5, 4, 60, 4, -7.0, 0.0),
}
LOO_BLOCKS = (1, 7, 8, 64)
LOO_CASES = [('k64_n256_a1', LOO_BLOCKS), ('k64_n62_a4', LOO_BLOCKS), ('k64_n62_a7', LOO_BLOCKS), ('k64_n62_a7b3', LOO_BLOCKS),
             ('k64_n32_a7b3', LOO_BLOCKS), ('k128_n64_a7', (8, 64))]
# (fit, keep): rows keep .. N leave the fit
FORGET_CASES = [('k64_n256_a1', 128), ('k64_n256_a1', 1), ('k64_n256_a4', 16), ('k64_n256_a7', 16), ('k64_n256_a7', 1),
                ('k64_n62_a7b3', 16), ('k64_n256_a7b3', 1), ('k128_n136_a7', 32), ('k128_n136_a7', 1), ('k40_n160_a7b3', 10)]
HARD_FORGET = ('k64_n256_a7', 1)        # lam_min(S) = 9.2e-9: the case of the bit-level claims
MILD_FORGET = ('k64_n256_a1', 128)
# (fit, n): the n rows after the fit's own join it
COND_CASES = [('k64_n1_a7b3', 255), ('k64_n16_a7b3', 46), ('k128_n4_a7', 132), ('k64_n256_a1', 64)]
# ENOTPD boundary: k copies of one fit row of leverage h give S = I - k c c^T (loo: I - H = I - h 1 1^T) the eigenvalue 1 - k h.  Every
# leverage of the N = 62 fits lies above 1/2 (62 rows determine 64 weights), so the pairs come from the N = 256 fit (h about K / N)
BOUNDARY_FIT = 'k64_n256_a1'
BOUNDARY_COPIES = (2, 3, 4, 5, 6, 7, 8)
# (fit, row, k): k copies of one fit row leave the fit, chosen (by a search over rows and k in float64) so that the LAST pivot of the
# Cholesky of S = I - k c c^T is the smallest one: what the statistic min M_ii^2 must not miss.  K = 64 and the padded diagonal of K = 40.
# Only alpha', the pivot, the joint density and lam_min are stored for them.  Kinds of their own (copies_*): with one row the error of c =
# phi Li^T itself, a cancelling sum, is what 1 / lam_min(S) multiplies, and the restatement's constants are 5 .. 300 instead of 0.1 .. 80.
# The pair below the ENOTPD boundary is a case of these kinds too
PIVOT_CASES = [('k64_n256_a7', 182, 2), ('k40_n160_a7b3', 121, 3)]
KINDS = ('loo_musd', 'loo_lev', 'loo_joint', 'forget_Li', 'forget_alpha', 'forget_pivot', 'forget_joint', 'cond_Li', 'cond_alpha', 'cond_Li_c', 'cond_alpha_c', 'copies_alpha', 'copies_pivot', 'copies_joint',
         'forget_resid', 'cond_resid', 'cond_resid_c', 'cond32_Li', 'cond32_alpha', 'cond32_resid')
PRINTED = ('loo_cw_mu', 'loo_cw_std')          # measured and stored beside C_REF, not asserted


def fkey(fit, keep):
    return 'forget/%s_keep%d' % (fit, keep)


def ckey(fit, n):
    return 'cond/%s_add%d' % (fit, n)


def pkey(fit, row, k):
    return 'pivot/%s_row%d_x%d' % (fit, row, k)


def lkey(fit, block):
    return 'loo/%s_b%d' % (fit, block)


def kappa(params):
    return float(np.log1p(np.exp(params[2])))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def shape_key(D, S, M):
    return 'data/%d_%d_%d' % (D, S, M)


def make_inputs():
    """{key: array} of every input the generator starts from: rows and targets per shape, parameters per fit"""
    from scfgp_amd import synth
    from tests import condition_ref
    out = {}
    rows = {}
    for fit, (D, S, M, N, a, b) in FITS.items():
        rows[(D, S, M)] = max(rows.get((D, S, M), 0), N + max([n for f, n in COND_CASES if f == fit] + [0]))
        out['fit/%s/params' % fit] = synth.make_params(SEED + M + 0x0202, D, S, M, abc=(a, b, -1.0))
    for (D, S, M), N in rows.items():
        _, X, y, _ = condition_ref.problem(D, S, M, N, 0)
        out[shape_key(D, S, M) + '/X'] = X; out[shape_key(D, S, M) + '/y'] = y.ravel()
    return out


def pack(L):
    """the lower triangle of a square matrix, row by row"""
    return np.asarray(L, np.float64)[np.tril_indices(L.shape[0])]


def unpack(v):
    K = int(round((np.sqrt(8 * v.size + 1) - 1) / 2))
    L = np.zeros((K, K)); L[np.tril_indices(K)] = v
    return L


class Fixture(object):
    """read access to the fixture (or to the dict the generator is filling)"""

    def __init__(self, data=None):
        self.d = np.load(FIXTURE) if data is None else data
        self.a = np.load(RESID_FIXTURE) if data is None else data

    def __getitem__(self, k):
        return self.a[k] if k.endswith('/A') else self.d[k]

    def fit(self, fit):
        """(D, S, M, N, params, X (N, D), y (N,), alpha (K, 1), Li (K, K))"""
        D, S, M, N, a, b = FITS[fit]
        return (D, S, M, N, self.d['fit/%s/params' % fit], np.ascontiguousarray(self.d[shape_key(D, S, M) + '/X'][:N]),
                np.ascontiguousarray(self.d[shape_key(D, S, M) + '/y'][:N]), self.d['fit/%s/alpha' % fit].reshape(-1, 1),
                unpack(self.d['fit/%s/Li' % fit]))

    def rows(self, fit, i0, i1):
        D, S, M = FITS[fit][:3]
        return (np.ascontiguousarray(self.d[shape_key(D, S, M) + '/X'][i0:i1]), np.ascontiguousarray(self.d[shape_key(D, S, M) + '/y'][i0:i1]))

    def cref(self):
        return dict((k, float(self.d['cref/' + k])) for k in KINDS + PRINTED)

    def admitted(self, fit, block, u=U64):
        return float(self.d[lkey(fit, block) + '/margin']) * (U64 / u) >= ADMIT


# ---- ratios: error / (u model) ----------------------------------------------------------------------------------------------------------
def _rel(d, x):
    return float(np.linalg.norm(d) / np.linalg.norm(x))


def residual(Li, A):
    """max |Li A Li^T - I| for the symmetric A given by its packed lower triangle, in the widest float numpy has here.  A is the rounding
    of the true A' = L S L^T, so the figure has a floor of u max(|Li||A||Li|^T): what the rounding of a perfect Li' to doubles costs too"""
    t = np.longdouble
    A = unpack(A); A = (A + np.tril(A, -1).T).astype(t)
    L = np.tril(np.asarray(Li, np.float64)).astype(t)
    return float(np.max(np.abs(L @ A @ L.T - np.eye(L.shape[0], dtype=t))))


def factor_ratios(fx, key, alpha, Li, model, u=U64):
    """dict(Li, alpha, resid) of an (alpha', Li') against the truth of forget / condition case `key`"""
    L0 = unpack(fx[key + '/Li']); a0 = fx[key + '/alpha'].ravel()
    Li = np.asarray(Li, np.float64); al = np.asarray(alpha, np.float64).ravel()
    nl = np.linalg.norm(L0); Lt = np.tril(Li)
    li = max(float(np.linalg.norm(Lt[i:i + TILE] - L0[i:i + TILE]) / nl) for i in range(0, L0.shape[0], TILE))
    return dict(Li=li / (u * model), alpha=_rel(al - a0, a0) / (u * model), resid=residual(Li, fx[key + '/A']) / (u * model))


def forget_ratios(fx, fit, keep, alpha, Li, pivot2, joint):
    key = fkey(fit, keep)
    model = 1.0 / float(fx[key + '/lam_min'])
    n = FITS[fit][3] - keep
    r = factor_ratios(fx, key, alpha, Li, model)
    p0 = float(fx[key + '/pivot2'])
    r = dict(forget_Li=r['Li'], forget_alpha=r['alpha'], forget_resid=r['resid'], forget_pivot=abs(pivot2 - p0) / p0 / (U64 * model),
             forget_joint=abs(float(np.sum(joint)) - float(fx[key + '/joint'])) / (n * U64 * model))
    return r


def boundary_case(fx):
    """(fit, row, k) of the copies just below the ENOTPD boundary"""
    return BOUNDARY_FIT, int(fx['boundary/rows'][0]), int(fx['boundary/copies'][0])


def pivot_ratios(fx, fit, row, k, alpha, pivot2, joint, key=None):
    key = key or pkey(fit, row, k)
    model = 1.0 / float(fx[key + '/lam_min'])
    a0 = fx[key + '/alpha'].ravel(); p0 = float(fx[key + '/pivot2'])
    return dict(copies_alpha=_rel(np.asarray(alpha, np.float64).ravel() - a0, a0) / (U64 * model), copies_pivot=abs(pivot2 - p0) / p0 / (U64 * model),
                copies_joint=abs(float(np.sum(joint)) - float(fx[key + '/joint'])) / (k * U64 * model))


def cond_admitted_f32(fx, fit, n):
    """scfgp_condition forms C^T C in the context's precision: in an fp32 context S keeps its unit eigenvalues only while eps32 K |S| is
    far below them -- the loo admission rule with S in place of I - H"""
    K = 2 * (FITS[fit][1] + FITS[fit][2])
    return float(fx[ckey(fit, n) + '/lam_min']) / (U32 * K * float(fx[ckey(fit, n) + '/lam_max'])) >= ADMIT


def cond_ratios(fx, fit, n, alpha, Li, u=U64):
    K = 2 * (FITS[fit][1] + FITS[fit][2])
    r = factor_ratios(fx, ckey(fit, n), alpha, Li, float(K), u)
    c = factor_ratios(fx, ckey(fit, n), alpha, Li, float(fx[ckey(fit, n) + '/lam_max']) / float(fx[ckey(fit, n) + '/lam_min']), u)
    return dict(cond_Li=r['Li'], cond_alpha=r['alpha'], cond_resid=r['resid'], cond_Li_c=c['Li'], cond_alpha_c=c['alpha'], cond_resid_c=c['resid'])


def cond32_ratios(fx, fit, n, alpha, Li):
    """an fp32 context's factors (C and C^T C formed in fp32) in units of eps32 cond(S): the kinds cond32_*, whose C_REF is the
    restatement's with tests/parity.apply32_model's products, over the cases where its Cholesky exists"""
    c = factor_ratios(fx, ckey(fit, n), alpha, Li, float(fx[ckey(fit, n) + '/lam_max']) / float(fx[ckey(fit, n) + '/lam_min']), U32)
    return dict(cond32_Li=c['Li'], cond32_alpha=c['alpha'], cond32_resid=c['resid'])


def loo_ratios(fx, fit, block, mu, sd, lev, sum_joint, u=U64):
    """worst constant over rows of mu / std (loo_musd: against sigma / (1 - lam_max); loo_cw_mu, loo_cw_std: the component-wise model), of
    the leverage, and the constant of the summed joint density"""
    key = lkey(fit, block)
    mu = np.asarray(mu, np.float64).ravel(); sd = np.asarray(sd, np.float64).ravel(); lev = np.asarray(lev, np.float64).ravel()
    dm = np.abs(mu - fx[key + '/mu']); ds = np.abs(sd - fx[key + '/std'])
    simple = fx[key + '/std'] / np.repeat(fx[key + '/gap'], block)[:mu.size]
    out = dict(loo_musd=float(np.max(np.maximum(dm, ds) / simple)) / u,
               loo_lev=float(np.max(np.abs(lev - fx['lev/%s/lev' % fit]) / fx['lev/%s/den_lev' % fit])) / u,
               loo_cw_mu=float(np.max(dm / fx[key + '/den_mu'])) / u, loo_cw_std=float(np.max(ds / fx[key + '/den_std'])) / u)
    if sum_joint is not None:
        out['loo_joint'] = abs(sum_joint - float(np.sum(fx[key + '/joint']))) / (u * float(np.sum(fx[key + '/den_joint'])))
    return out


def loo_models(Phi, C, PhiAbsLi, alpha, y, G, sd, e, t2, one_minus_lmax, kap, K):
    """per-row denominators of one block from (roundings of) its true quantities: dict(den_mu, den_std, den_lev) and the block's
    den_joint"""
    b = C.shape[0]
    E = np.abs(C) @ np.abs(C).T + np.eye(b)
    aG = np.abs(G)
    den_mu = aG @ ((K + b) * (E @ np.abs(e)) + (K + 2) * (np.abs(Phi) @ np.abs(alpha).ravel() + np.abs(y)))
    den_std = sd / (2.0 * np.diag(G)) * (K + b) * np.diag(aG @ E @ aG)
    den_lev = 2.0 * np.sum(np.abs(C) * PhiAbsLi, axis=1) + np.sum(C * C, axis=1)
    return dict(den_mu=den_mu, den_std=den_std, den_lev=den_lev), (t2 / kap + b) / one_minus_lmax


# ---- the numpy restatements, and their mutants -------------------------------------------------------------------------------------------
# c36: C keeps 36 bits (five digits lost in the product); pivot_1e12: the final pivot is off by 1e-12 relative (an rsq seed short of a
# Newton step) -- the subtle ones, far inside today's fixed 1e-9
# li_small_row: the row of Li' with the smallest norm is off by 1e-4 relative -- invisible in a norm that the large rows dominate
MUTANTS = ('c32', 'pivot_term', 'r32', 'alpha_li_new', 'min_before', 'c36', 'pivot_1e12', 'li_small_row')


def _f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def _c36(x):
    m, e = np.frexp(x)
    return np.ldexp(np.round(m * 2.0 ** 36) / 2.0 ** 36, e)


def _cholesky(Sm, mutant=None):
    """lower Cholesky factor, row by row; `pivot_term`: the last inner-product term is missing from the final pivot"""
    K = Sm.shape[0]
    Mc = np.zeros_like(Sm)
    for i in range(K):
        for j in range(i):
            Mc[i, j] = (Sm[i, j] - Mc[i, :j] @ Mc[j, :j]) / Mc[j, j]
        stop = i - 1 if (mutant == 'pivot_term' and i == K - 1) else i
        d = Sm[i, i] - Mc[i, :stop] @ Mc[i, :stop]
        if not d > 0.0:
            raise np.linalg.LinAlgError('not positive definite')
        Mc[i, i] = np.sqrt(d) * (1.0 + 1e-12 if (mutant == 'pivot_1e12' and i == K - 1) else 1.0)
    return Mc


def update_np(Xr, yr, alpha, Li, params, S, M, sign, mutant=None):
    """forget (sign -1) / condition (sign +1) restated once more with the seams the mutants cut at: dict(alpha, Li, pivot2, joint)"""
    Xr = np.asarray(Xr, np.float64); yr = np.asarray(yr, np.float64).reshape(-1, 1)
    Li = np.tril(np.asarray(Li, np.float64)); alpha = np.asarray(alpha, np.float64).reshape(-1, 1)
    Phi = O.feature_map(Xr, params, Xr.shape[1], S, M)
    C = Phi @ Li.T
    if mutant in ('c32', 'c36'):
        C = _f32(C) if mutant == 'c32' else _c36(C)
    f = Phi @ alpha
    r = yr - (_f32(f) if mutant == 'r32' else f)
    if mutant == 'apply32':                                         # what an fp32 context forms: C and C^T C by fp32 products
        C = (np.asarray(Phi, np.float32) @ np.asarray(Li.T, np.float32)).astype(np.float64)
        G = (np.asarray(C.T, np.float32) @ np.asarray(C, np.float32)).astype(np.float64)
    else:
        G = C.T @ C
    Sm = np.eye(Li.shape[0]) + sign * G
    Mc = _cholesky(Sm, mutant)
    Li_new = np.tril(np.linalg.solve(Mc, Li))
    if mutant == 'li_small_row':
        Li_new[np.argmin(np.linalg.norm(Li_new, axis=1))] *= 1.0 + 1e-4
    w = np.linalg.solve(Mc, C.T @ r)
    gamma = np.linalg.solve(Mc.T, w)
    alpha_new = alpha + sign * ((Li_new if mutant == 'alpha_li_new' else Li).T @ gamma)
    kap = kappa(params)
    d = np.diag(Mc)
    n = Xr.shape[0]
    joint = -0.5 * (((r.T @ r).item() + (w.T @ w).item()) / kap + n * np.log(2 * np.pi * kap) - 2.0 * np.sum(np.log(d)))
    return dict(alpha=alpha_new, Li=Li_new, pivot2=float(np.min(d[:-1] if mutant == 'min_before' else d)) ** 2, joint=joint)


def loo_np(X, y, alpha, Li, params, S, M, block, mutant=None):
    """tests/loo_ref.loo with the seams of the mutants `c32` and `r32`: dict(mu, std, lev, joint (nblocks,))"""
    from tests import loo_ref
    if mutant is None:
        return loo_ref.loo(X, y, alpha, Li, params, S, M, block=block)
    X = np.asarray(X, np.float64); y = np.asarray(y, np.float64).ravel()
    n = X.shape[0]
    Li = np.tril(np.asarray(Li, np.float64)); alpha = np.asarray(alpha, np.float64).reshape(-1, 1)
    kap = kappa(params)
    mu = np.empty(n); sd = np.empty(n); lev = np.empty(n); joint = []
    for i0, i1 in loo_ref.blocks(n, block):
        Phi = O.feature_map(X[i0:i1], params, X.shape[1], S, M)
        C = Phi @ Li.T
        if mutant in ('c32', 'c36'):
            C = _f32(C) if mutant == 'c32' else _c36(C)
        elif mutant == 'apply32':                                   # the C an fp32 context holds (tests/parity.apply32_model)
            C = (np.asarray(Phi, np.float32) @ np.asarray(Li.T, np.float32)).astype(np.float64)
        f = (Phi @ alpha).ravel()
        r = y[i0:i1] - (_f32(f) if mutant == 'r32' else f)
        H = C @ C.T
        R = np.linalg.cholesky(np.eye(i1 - i0) - H)
        W = np.linalg.inv(R)
        t = W @ r
        mu[i0:i1] = y[i0:i1] - W.T @ t
        sd[i0:i1] = np.sqrt(kap * np.sum(W * W, axis=0))
        lev[i0:i1] = np.diag(H)
        joint.append(-0.5 * (t @ t / kap + (i1 - i0) * np.log(2 * np.pi * kap) - 2.0 * np.sum(np.log(np.diag(R)))))
    return dict(mu=mu, std=sd, lev=lev, joint=np.array(joint))


def restate_forget(fx, fit, keep, mutant=None):
    D, S, M, N, params, X, y, alpha, Li = fx.fit(fit)
    if mutant is None:
        from tests import forget_ref
        o = forget_ref.forget(X[keep:], y[keep:], alpha, Li, params, S, M)
        return dict(alpha=o['alpha'], Li=o['Li'], pivot2=float(o['stats'][5]), joint=float(o['stats'][4]))
    return update_np(X[keep:], y[keep:], alpha, Li, params, S, M, -1.0, mutant)


def restate_pivot(fx, fit, row, k, mutant=None):
    D, S, M, N, params, X, y, alpha, Li = fx.fit(fit)
    Xo = np.repeat(X[row:row + 1], k, axis=0); yo = np.repeat(y[row:row + 1], k)
    if mutant is None:
        from tests import forget_ref
        o = forget_ref.forget(Xo, yo, alpha, Li, params, S, M)
        return dict(alpha=o['alpha'], Li=o['Li'], pivot2=float(o['stats'][5]), joint=float(o['stats'][4]))
    return update_np(Xo, yo, alpha, Li, params, S, M, -1.0, mutant)


def restate_cond(fx, fit, n, mutant=None):
    D, S, M, N, params, X, y, alpha, Li = fx.fit(fit)
    Xn, yn = fx.rows(fit, N, N + n)
    if mutant is None:
        from tests import condition_ref
        a, L = condition_ref.condition(Xn, yn, alpha, Li, params, S, M)
        return dict(alpha=a, Li=L)
    return update_np(Xn, yn, alpha, Li, params, S, M, 1.0, mutant)


def restate_loo(fx, fit, block, mutant=None):
    D, S, M, N, params, X, y, alpha, Li = fx.fit(fit)
    return loo_np(X, y, alpha, Li, params, S, M, block, mutant)


def all_ratios(fx, forget=restate_forget, cond=restate_cond, loo=restate_loo, pivot=restate_pivot, u_loo=U64):
    """{case key: {kind: constant}} of an implementation (the restatements by default) over every admitted case"""
    out = {}
    for fit, keep in FORGET_CASES:
        o = forget(fx, fit, keep)
        out[fkey(fit, keep)] = forget_ratios(fx, fit, keep, o['alpha'], o['Li'], o['pivot2'], o['joint'])
    for fit, row, k in PIVOT_CASES:
        o = pivot(fx, fit, row, k)
        out[pkey(fit, row, k)] = pivot_ratios(fx, fit, row, k, o['alpha'], o['pivot2'], o['joint'])
    fit, row, k = boundary_case(fx)
    o = pivot(fx, fit, row, k)
    out['boundary'] = pivot_ratios(fx, fit, row, k, o['alpha'], o['pivot2'], o['joint'], key='boundary')
    for fit, n in COND_CASES:
        o = cond(fx, fit, n)
        out[ckey(fit, n)] = cond_ratios(fx, fit, n, o['alpha'], o['Li'])
    for fit, blocks in LOO_CASES:
        for block in blocks:
            if fx.admitted(fit, block, u_loo):
                o = loo(fx, fit, block)
                out[lkey(fit, block)] = loo_ratios(fx, fit, block, o['mu'], o['std'], o['lev'], float(np.sum(o['joint'])), u_loo)
    return out


def cond32_reference(fx):
    """{case key: cond32 constants} of the restatement with an fp32 context's products, where its Cholesky exists"""
    out = {}
    for fit, n in COND_CASES:
        try:
            o = restate_cond(fx, fit, n, mutant='apply32')
        except np.linalg.LinAlgError:
            continue
        out[ckey(fit, n)] = cond32_ratios(fx, fit, n, o['alpha'], o['Li'])
    return out


def worst(ratios):
    """{kind: (constant, case key)} of the largest constant per kind"""
    out = {}
    for key, r in ratios.items():
        for kind, v in r.items():
            if kind not in out or not v <= out[kind][0]:
                out[kind] = (float(v), key)
    return out


def failures(ratios, cref, factor):
    return ['%s %s: %.3g > %g x %.3g' % (key, kind, v, factor, cref[kind]) for key, r in sorted(ratios.items()) for kind, v in r.items()
            if kind in cref and not v <= factor * cref[kind]]


def fmt(w):
    return ' '.join('%s=%.3g' % (k, v[0]) for k, v in sorted(w.items()))
