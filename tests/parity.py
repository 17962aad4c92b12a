"""
Block-level comparison of the HIP path with the CPU oracle (not a test, not a conftest: a helper of tests/test_parity_blocks.py,
tests/test_gpu_stage_tiles.py and the GPU parity tests).

A norm over a whole output cannot see one wrong tile, row block or flush: the gradient's norm is dominated by its noise entry
d/da, and the phase entries d/dl_P, d/dP are exactly zero (a phase rotates each cos / sin pair, under which the NLML is
invariant).  So every check here is per block:
  gradient      a, b, c each relative; l_F and each group of 32 frequencies of r_F as ||D_B|| <= beta ||g0_B|| + tau ||scale_B||;
                every entry of l_F, r_F, l_P, P as |D_i| <= beta |g0_i| + tau scale_i, scale = the oracle's abs-sum scale
                (oracle.value_and_grad(..., with_scale=True)): for l_P and P "zero to within tau of its abs-sum"
  alpha, Li     per 64-entry tile of alpha / 64-row block of Li: ||D_t|| <= beta ||x0_t|| + tau ||x0||
  predict       every row: |D mu_t| <= eps sigma0_t and |D sigma_t| <= eps sigma0_t
  stages        worst normalised error |X - X_ref| / (|A|^T |B|) per tile of the kernel's own tiling, against an a-priori bound
                gamma_{L+1} u32 (+ u32 per operand rounded to fp32 on the way in, + u32 for an fp32 output) + gamma_n u64
"""
import numpy as np

from oracle import scfgp_oracle as O
from tests.f16x3_stage_ref import block_max, normalised

GROUP = 32                  # r_F frequencies per group
TILE = 64                   # alpha tile / Li row block: the apply launch's column-tile width
U32 = 2.0 ** -24
U64 = 2.0 ** -53

# (beta, tau) of the gradient, rho of a, b, c each, (beta, tau) of alpha and of Li, eps of predict.  fp64: the oracle's two
# restatements agree to 1.3e-13 of the abs-sum scale and 3.5e-14 relative in a, b, c (tests/test_parity_blocks.py); tau is 4x the
# GPU's worst phase entry, 1.6e-11 of its abs-sum at N = 1000, D = 5, S = 64, M = 3 (Abar's error there is cond(A) u64).  fp32: set so that the worst ratio the GPU tests measure
# against the oracle is <= 0.25 (profiles/r08_parity_blocks.md), except tau and rho_a: the seeded random
# shapes of fp32 mode reach 0.81 (phase entries) and 0.43 (a), and a 4x margin there would stop the CPU tier catching a 4 % change
# of one r_F group by 10x.  The worst cases are f16x3 at K <= 256 with the fp16 Gram (alpha,
# Li, predict): there the Gram's error is the three-term split's floor (2^-22 |a||b| per term, tests/f16x3_stage_ref.py), 6.6x
# fp32 mode's at K = 128 and N = 3000 (3.7e-7 against 5.6e-8 of |Phi|^T |Phi|), and alpha / Li carry it times cond(A) = 3e4.
# b: 4.5e-4 relative at worst (its closed form 2 tr(Abar G) + ... cancels), the phase entries 2.9e-6 of their abs-sum
TOL = {
    'f64': dict(beta=1e-9, tau=7e-11, rho=(1e-9, 1e-9, 1e-9), vbeta=1e-9, vtau=1e-10, lbeta=1e-9, ltau=1e-10, eps=1e-9),
    'f32': dict(beta=5e-4, tau=1.2e-5, rho=(1e-5, 2e-3, 1e-5), vbeta=8e-4, vtau=8e-5, lbeta=7e-4, ltau=7e-5, eps=1.5e-6),
}
TOL['f16x3'] = TOL['f32']   # the mode claims fp32-grade parity


def _tol(dtype):
    """a row of TOL by its name, or a row given as a dict"""
    return dtype if isinstance(dtype, dict) else TOL[dtype]


# ---- layout ------------------------------------------------------------------------------------------------------------------
def layout(D, S, M):
    """flat indices of (a, b, c, l_F, r_F, l_P, P), read off oracle.unpack_params applied to the index vector itself"""
    n = O.num_params(D, S, M)
    a, b, c, l_F, r_F, F, l_FC, FC = O.unpack_params(np.arange(n, dtype=np.float64), D, S, M)
    l_P = np.rint(l_FC.ravel() + l_F.mean(0)).astype(np.int64)
    P = np.rint(FC.ravel() + F.mean(0)).astype(np.int64)
    assert np.array_equal(P, l_P[-1] + 1 + np.arange(M))
    return dict(a=0, b=1, c=2, l_F=l_F.astype(np.int64).ravel(), r_F=r_F.astype(np.int64), l_P=l_P, P=P)


def rf_groups(M):
    """frequency ranges of the r_F groups: GROUP consecutive rows of r_F (M x S), the last one ragged"""
    e = list(range(0, M, GROUP)) + [M]
    return list(zip(e[:-1], e[1:]))


def _mixed(d, x0, s, beta, tau):
    """||d|| / (beta ||x0|| + tau ||s||), 0 where d is exactly 0"""
    num = np.linalg.norm(d)
    den = beta * np.linalg.norm(x0) + tau * np.linalg.norm(s)
    return 0.0 if num == 0 else (num / den if den > 0 else np.inf)


# ---- gradient ----------------------------------------------------------------------------------------------------------------
def grad_ratios(g, g0, scale, D, S, M, dtype):
    """measured / bound of every gradient check (> 1 fails): a, b, c, l_F, the worst r_F group, the worst entry of l_F / r_F,
    the worst phase entry"""
    t = _tol(dtype)
    g = np.asarray(g, np.float64).ravel(); g0 = np.asarray(g0, np.float64).ravel()
    sc = np.concatenate((np.zeros(3), np.asarray(scale, np.float64).ravel()))
    assert g.shape == g0.shape == sc.shape
    L = layout(D, S, M)
    d = g - g0
    out = {}
    for k, rho in zip(('a', 'b', 'c'), t['rho']):
        i = L[k]
        out[k] = 0.0 if d[i] == 0 else abs(d[i]) / (rho * abs(g0[i]))
    lf = L['l_F']
    out['l_F'] = _mixed(d[lf], g0[lf], sc[lf], t['beta'], t['tau'])
    out['r_F'] = max(_mixed(d[ix], g0[ix], sc[ix], t['beta'], t['tau'])
                     for ix in (L['r_F'][f0:f1].ravel() for f0, f1 in rf_groups(M)))
    ent = lambda ix: float((np.abs(d[ix]) / (t['beta'] * np.abs(g0[ix]) + t['tau'] * sc[ix])).max())
    out['entry'] = ent(np.concatenate((lf, L['r_F'].ravel())))
    out['phase'] = ent(np.concatenate((L['l_P'], L['P'])))
    return out


def check_grad(g, g0, scale, D, S, M, dtype):
    r = grad_ratios(g, g0, scale, D, S, M, dtype)
    assert max(r.values()) <= 1.0, ('gradient block outside its bound', dtype, r)
    return r


# ---- alpha, Li ---------------------------------------------------------------------------------------------------------------
def alpha_ratio(al, al0, dtype):
    t = _tol(dtype)
    al = np.asarray(al, np.float64).ravel(); al0 = np.asarray(al0, np.float64).ravel()
    return max(_mixed(al[i:i + TILE] - al0[i:i + TILE], al0[i:i + TILE], al0, t['vbeta'], t['vtau'])
               for i in range(0, len(al0), TILE))


def li_ratio(Li, Li0, dtype):
    t = _tol(dtype)
    Li = np.asarray(Li, np.float64); Li0 = np.asarray(Li0, np.float64)
    return max(_mixed(Li[i:i + TILE] - Li0[i:i + TILE], Li0[i:i + TILE], Li0, t['lbeta'], t['ltau'])
               for i in range(0, Li0.shape[0], TILE))


def check_alpha(al, al0, dtype):
    r = alpha_ratio(al, al0, dtype)
    assert r <= 1.0, ('alpha tile outside its bound', dtype, r)
    return r


def check_li(Li, Li0, dtype):
    r = li_ratio(Li, Li0, dtype)
    assert r <= 1.0, ('Li row block outside its bound', dtype, r)
    return r


# ---- predict -----------------------------------------------------------------------------------------------------------------
def predict_ratio(mu, sd, mu0, sd0, dtype):
    """worst over rows of max(|D mu_t|, |D sigma_t|) / (eps sigma0_t)"""
    e = _tol(dtype)['eps']
    mu = np.asarray(mu, np.float64).ravel(); mu0 = np.asarray(mu0, np.float64).ravel()
    sd = np.asarray(sd, np.float64).ravel(); sd0 = np.asarray(sd0, np.float64).ravel()
    return float((np.maximum(np.abs(mu - mu0), np.abs(sd - sd0)) / (e * sd0)).max())


def check_predict(mu, sd, mu0, sd0, dtype):
    r = predict_ratio(mu, sd, mu0, sd0, dtype)
    assert r <= 1.0, ('predictive row outside its bound', dtype, r)
    return r


def oracle_all(X, y, params, S, M, Xs=None):
    """the oracle's (cost, grad, alpha, Li, scale) and, given Xs, its (mu, std) from its own alpha and Li"""
    c0, g0, a0, L0, sc = O.value_and_grad(X, y, params, S, M, with_scale=True)
    out = dict(cost=c0, grad=g0, alpha=a0, Li=L0, scale=sc)
    if Xs is not None:
        out['mu'], out['std'] = O.predict(Xs, a0, L0, params, S, M)
    return out


def check_all(res, ref, D, S, M, dtype):
    """check_grad / check_alpha / check_li of an evaluation's (cost, grad, alpha, Li) against oracle_all's dict"""
    cost, grad, alpha, Li = res[:4]
    r = dict(check_grad(grad, ref['grad'], ref['scale'], D, S, M, dtype))
    r['alpha'] = check_alpha(alpha, ref['alpha'], dtype)
    r['Li'] = check_li(Li, ref['Li'], dtype)
    return r


def oracle_check(res, X, y, params, S, M, dtype, alpha_li=True, label=''):
    """check_grad (and check_alpha / check_li) of an evaluation's (cost, grad, alpha, Li) against the oracle on the same inputs;
    prints the ratios"""
    X = np.asarray(X); D = X.shape[1]
    ref = oracle_all(X, y, params, S, M)
    r = dict(check_grad(res[1], ref['grad'], ref['scale'], D, S, M, dtype))
    if alpha_li:
        r['alpha'] = check_alpha(res[2], ref['alpha'], dtype)
        r['Li'] = check_li(res[3], ref['Li'], dtype)
    print('%s %s (N %d D %d S %d M %d) blocks: %s' % (label, dtype, X.shape[0], D, S, M, fmt(r)))
    return r


def fmt(r):
    return ' '.join('%s %.2g' % kv for kv in r.items())


# ---- stages ------------------------------------------------------------------------------------------------------------------
def gamma(n, u):
    return n * u / (1 - n * u)


def bound32(L, n64=1, rounded=0, out32=False):
    """a-priori bound of the normalised error of a product whose fp32 chains of length L are added into fp64 (n64 terms of that
    sum); `rounded` operands rounded to fp32 on the way in; an fp32 output"""
    return gamma(L + 1, U32) + rounded * U32 + (U32 if out32 else 0.0) + gamma(n64, U64)


def bound64(n):
    return gamma(n, U64)


def edges(n, step):
    return list(range(0, n, step)) + [n]


def stage_error(X, X_ref, scale_abs, row_edges, col_edges):
    """worst normalised error |X - X_ref| / scale_abs per (row block, column block)"""
    return block_max(normalised(X, X_ref, scale_abs), row_edges, col_edges)


# ---- a numpy fp32 model of the products (CPU tests: a correct result to hold the stage bounds against) ---------------------------
def gram32_model(A, B=None, chain=4096):
    """A^T B (B = A) with fp32 chains of `chain` rows, each added into fp64"""
    A32 = np.asarray(A, np.float32); B32 = A32 if B is None else np.asarray(B, np.float32)
    out = np.zeros((A32.shape[1], B32.shape[1]))
    for r0 in range(0, A32.shape[0], chain):
        out += (A32[r0:r0 + chain].T @ B32[r0:r0 + chain]).astype(np.float64)
    return out


def apply32_model(A, B):
    """A B of fp32 operands, fp32 accumulation over k, fp32 output"""
    return (np.asarray(A, np.float32) @ np.asarray(B, np.float32)).astype(np.float64)
