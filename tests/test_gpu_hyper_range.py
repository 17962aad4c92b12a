"""GPU tier of the hyper-parameter range tests: the O(P) kernels either side of the sweeps (kernels_params.hip: scal_kernel, the penalty
statistics, fbar / grad_tail / lbar with their rank-S branches, finalize_kernel) through the public API, away from (a, b, c) = (-1, 0, -1).

  kappa, s         element by element over the CPU tier's grids, read back through predict with factors that isolate them, against
                   double-double mpmath values; allowance 4 x the CPU tier's measured error of the correct restatement
  the objective    cost, gradient, alpha, Li and predict at a star and four corners of (a, b, c) against mpmath truths of the whole
                   objective (tests/golden/hyper_kats.npz); allowance max(the fp64 tolerance of test_ragged_and_degenerate_shapes,
                   8 x what float64 rounding costs the oracle at that point), alpha and Li to C_KSTAGE K u64 cond(A)
  R_PEN            debug_read('scalars') on the CPU tier's edge rows, against mpmath
  fp32 mode        the c axis under tests/parity.py's fp32 row
  entry points     predict, predict_cov (noise on the diagonal) and acquire (predictive sigma) at the ends of c, under their own bounds
  std = 0          a non-finite cost, then a correct evaluation on the same context
No mpmath is needed here.

Measured on the device (MI355X), worst over each test:
  kappa            |std^2 / kappa - 1| 3.2e-16 (c = 16.25), fp64 and fp32 context alike; bound 8.4e-16
  s                2.3e-16 (M = 300, b = 4.625), 1.8e-16 (M = 5); bound 9.6e-16
  the objective    measured / allowed: cost 0.049, a 0.0037, b 0.088, c 0.0029, l_F 0.0017, r_F 0.0014, l_P 2.3e-4, P 3.1e-4, alpha 0.17
                   (cond(A) = 1.8), Li 0.038, predict 6.1e-6
  R_PEN            error / allowed at most 0.17 ((64, 2, 70), sig_large: 9.3e-10 of 3.8e6)
With alpha formed as B g, B = A^-1 (the library before this test), the same points gave cost 14, b 51, l_P 12, P 3.5, r_F 2.5 at
a = -7 (cond(A) = 3e8), b 1.2 at a = -4 and cost 1.6 at b = 4: g^T alpha missed |Li g|^2 by cond(A) u, times e^{-2a}; with
kappa = log(1 + e^c) the kappa test failed from c = -14 down (0.25 at c = -35.75) and the cost at c = -30 by 1e7 allowances."""
import os

import numpy as np
import pytest

from oracle import scfgp_oracle as O
from scfgp_amd import synth
from tests import acquire_ref as A
from tests import hyper_ref as H
from tests import parity as PB
from tests import pred_cov_ref as R
from tests.test_gpu_stage_tiles import C_KSTAGE

pytestmark = pytest.mark.gpu

KATS = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'hyper_kats.npz'))
N = 257
SHAPES = {'d3': (3, 2, 5), 'd20': (20, 2, 5)}
R_PEN = 7                                                       # slot of the penalty in the device scalars (common.h)
BLOCKS = ('cost', 'a', 'b', 'c', 'l_F', 'r_F', 'l_P', 'P')     # columns of the fixture's `ens`

# 4 x the CPU tier's figure: the device's exp / log1p against numpy's, and the sqrt and the square on the way through predict
KAPPA_BOUND = 4 * H.MEASURED_SCALAR_ERR['kappa']
S_BOUND = 4 * H.MEASURED_SCALAR_ERR['s']
# floors: test_ragged_and_degenerate_shapes' fp64 tolerance (cost 1e-10 max(1, |cost|), gradient 1e-8 relative); the phase blocks, whose
# truth is 0, are read against their abs-sum scale, where tests/parity.py's fp64 row allows tau
COST_FLOOR, BLOCK_FLOOR, PHASE_FLOOR = 1e-10, 1e-8, PB.TOL['f64']['tau']
ENS_FACTOR = 8                                                  # the device sums in another order than any of the four permutations


def _engine(D, S, M, dtype='f64', **opts):
    from scfgp_amd.engine import HipEngine
    e = HipEngine(D, S, M, dtype=dtype)
    for k, v in opts.items():
        e.set_option(k, v)
    return e


def _dd_rel(x, hi, lo):
    """x / (hi + lo) - 1 without rounding the truth to one double"""
    return ((x - hi) - lo) / hi


# ---- kappa and s, element by element ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_kappa_through_predict(dtype):
    """alpha = 0, Li = 0: std = sqrt(kappa) exactly, in both contexts (the scalars are fp64 in every mode)"""
    D, S, M = 3, 2, 5
    K = 2 * (S + M)
    eng = _engine(D, S, M, dtype)
    params = synth.make_params(0x5CF6C001, D, S, M, abc=(-1.0, 0.0, -1.0))
    Xs = synth.make_X(0x5CF6C002, 3, D)
    cs, (hi, lo) = KATS['grid/c'], KATS['grid/kappa']
    assert cs.min() == -700 and cs.max() == 700 and (np.abs(cs) <= 36).sum() == H.C_GRID.size
    sd = np.empty(cs.size)
    for i, c in enumerate(cs):
        params[2] = c
        eng.set_params(params)
        mu, s3 = eng.predict(Xs, np.zeros((K, 1)), np.zeros((K, K)))
        assert (s3 == s3[0]).all() and (mu == 0).all()
        sd[i] = s3[0]
    eng.close()
    dense = np.abs(cs) <= 36
    err = np.abs(_dd_rel(sd * sd, hi, lo))
    worst = int(np.argmax(np.where(dense, err, 0)))
    print('kappa %s: worst |std^2 / kappa - 1| = %.2e at c = %g (bound %.2e)' % (dtype, err[worst], cs[worst], KAPPA_BOUND))
    assert (err[dense] <= KAPPA_BOUND).all(), [(c, e) for c, e in zip(cs[dense], err[dense]) if e > KAPPA_BOUND][:8]
    order = np.argsort(cs)
    assert np.isfinite(sd).all() and (sd > 0).all() and (np.diff(sd[order]) > 0).all()        # c = +-100, +-700 included


@pytest.mark.parametrize('M', H.M_GRID)
def test_s_through_predict(M):
    """l_F = r_F = 0 and all phases 0: every cos column is s; alpha = e_0, Li = 0: mu = s = e^b sqrt(2 / M)"""
    D, S = 3, 2
    K = 2 * (S + M)
    eng = _engine(D, S, M)
    params = np.zeros(O.num_params(D, S, M)); params[0] = -1.0; params[2] = -1.0
    Xs = synth.make_X(0x5CF6C003, 3, D)
    alpha = np.zeros((K, 1)); alpha[0] = 1.0
    bs, (hi, lo) = KATS['grid/b'], KATS['grid/s%d' % M]
    got = np.empty(bs.size)
    for i, b in enumerate(bs):
        params[1] = b
        eng.set_params(params)
        mu, _ = eng.predict(Xs, alpha, np.zeros((K, K)))
        assert (mu == mu[0]).all()
        got[i] = mu[0, 0]
    eng.close()
    err = np.abs(_dd_rel(got, hi, lo))
    print('s M = %d: worst relative error %.2e at b = %g (bound %.2e)' % (M, err.max(), bs[int(np.argmax(err))], S_BOUND))
    assert (err <= S_BOUND).all()


# ---- the objective at every stored point ----------------------------------------------------------------------------------------------
def _slices(D, S, M):
    o, out = 3, {'a': slice(0, 1), 'b': slice(1, 2), 'c': slice(2, 3)}
    for k, n in (('l_F', D * S), ('r_F', M * S), ('l_P', S), ('P', M)):
        out[k] = slice(o, o + n); o += n
    return out


def allowances(name, ip):
    """block -> allowance of the point: max(floor, 8 x the oracle's own worst error over four row permutations)"""
    ens = KATS[name + '/ens'][ip]
    cost = KATS[name + '/cost'][ip]
    out = {'cost': max(COST_FLOOR * max(1.0, abs(cost)), ENS_FACTOR * ens[0])}
    for j, k in enumerate(BLOCKS[1:], 1):
        out[k] = max(PHASE_FLOOR if k in ('l_P', 'P') else BLOCK_FLOOR, ENS_FACTOR * ens[j])
    return out


def point_ratios(name, ip, res, K):
    """measured / allowed of (cost, grad, alpha, Li) against the truths of point ip"""
    D, S, M = SHAPES[name]
    cost, grad, alpha, Li = res
    al = allowances(name, ip)
    g0 = KATS[name + '/grad'][ip]
    sc = np.concatenate((np.zeros(3), KATS[name + '/scale'][ip]))
    d = np.asarray(grad, np.float64).ravel() - g0
    r = {'cost': abs(float(cost) - KATS[name + '/cost'][ip]) / al['cost']}
    for k, sl in _slices(D, S, M).items():
        ref = sc[sl] if k in ('l_P', 'P') else g0[sl]
        r[k] = np.linalg.norm(d[sl]) / np.linalg.norm(ref) / al[k]
    bK = C_KSTAGE * K * PB.U64 * KATS[name + '/cond'][ip]
    a0, L0 = KATS[name + '/alpha'][ip], KATS[name + '/Li'][ip]
    r['alpha'] = np.linalg.norm(np.asarray(alpha).ravel() - a0) / np.linalg.norm(a0) / bK
    r['Li'] = np.linalg.norm(np.asarray(Li) - L0) / np.linalg.norm(L0) / bK
    return r


def _lrb_rule(eng, S, lowrank_bwd):
    """the host rule (api_ctx.h: want_lrb) from dims(): does the gradient run the TZ / XU branches?"""
    d = eng.dims()
    Sp = -(-(S + 1) // 16) * 16
    fits = Sp < d['Dp'] and d['Jp'] + -(-S // 64) * 64 <= d['Kp']
    return fits and (lowrank_bwd == 1 or (lowrank_bwd < 0 and d['Dp'] >= 4 * Sp))


def predict_ratio(mu, sd, mu0, sd0, scale):
    """tests/parity.py's predict row with its eps, each quantity on its own scale: |D sigma_t| <= eps sigma0_t, and |D mu_t| <=
    eps (sigma0_t + (|phi_t| . |alpha|)): far down the c axis sigma is 1e-7 of mu, and mu's rounding does not shrink with kappa"""
    e = PB.TOL['f64']['eps']
    mu = np.asarray(mu).ravel(); mu0 = np.asarray(mu0).ravel()
    return float(max((np.abs(sd - sd0) / (e * sd0)).max(), (np.abs(mu - mu0) / (e * (sd0 + scale))).max()))


# d3: the dense projection.  d20: Sp < Dp, the projection runs through the S columns; the rank-S form of the GRADIENT (TZ / XU) needs room
# for U in Phibar, Jp + round_up(S, 64) <= Kp, which K = 14 does not give -- test_penalty_edge_rows_on_the_device takes those branches
@pytest.mark.parametrize('name', ['d3', 'd20'])
def test_objective_at_every_point(name):
    D, S, M = SHAPES[name]
    K = 2 * (S + M)
    X, y, Xs, params = (KATS['%s/%s' % (name, k)] for k in ('X', 'y', 'Xs', 'params'))
    assert X.shape == (N, D) and N % 256 == 1
    eng = _engine(D, S, M, 'f64')
    assert (-(-(S + 1) // 16) * 16 < eng.dims()['Dp']) == (name == 'd20')
    assert not _lrb_rule(eng, S, -1) and not _lrb_rule(eng, S, 1)
    eng.set_params(params); eng.set_data(X, y)
    bad = []
    for ip, abc in enumerate(KATS[name + '/abc']):
        p = params.copy(); p[:3] = abc
        eng.set_params(p)
        res = eng.eval(want_grad=True)
        r = point_ratios(name, ip, res, K)
        a0 = KATS[name + '/alpha'][ip]
        mu, sd = eng.predict(Xs, a0, KATS[name + '/Li'][ip])
        r['predict'] = predict_ratio(mu, sd, KATS[name + '/mu'][ip], KATS[name + '/std'][ip],
                                     np.abs(O.feature_map(Xs, p, D, S, M)) @ np.abs(a0))
        print('%s (a, b, c) = (%g, %g, %g) cond %.1e measured / allowed: %s' % (
            name, abc[0], abc[1], abc[2], KATS[name + '/cond'][ip], PB.fmt(r)), flush=True)
        bad += [(tuple(float(v) for v in abc), k, float(v)) for k, v in r.items() if not v <= 1.0]
    eng.close()
    assert not bad, bad


def test_the_old_kappa_line_would_have_failed():
    """vacuity guard: at c = -20 the stored truths differ from an evaluation with float64's log(1 + e^c) by more than the allowances"""
    i20 = int(np.argmin(np.abs(KATS['grid/c'] + 20.0)))
    hi, lo = KATS['grid/kappa'][:, i20]
    assert abs(_dd_rel(np.log(1.0 + np.exp(-20.0)), hi, lo)) > 10 * KAPPA_BOUND
    seen = 0
    for name in SHAPES:
        for ip, abc in enumerate(KATS[name + '/abc']):
            if abc[2] > -20.0:
                continue
            seen += 1
            assert abs(KATS[name + '/cost_plain'][ip] - KATS[name + '/cost'][ip]) > 2 * allowances(name, ip)['cost'], (name, abc)
            sd0, sd1 = KATS[name + '/std'][ip], KATS[name + '/std_plain'][ip]
            assert (np.abs(sd1 - sd0) > 2 * PB.TOL['f64']['eps'] * sd0).all(), (name, abc)
    assert seen == 8                                            # c = -20 and the three points at c = -30, per shape


# ---- R_PEN on the edge rows ---------------------------------------------------------------------------------------------------------
def _pen_allowance(l_F, r_F, S, M):
    """absolute allowance of R_PEN: 4 x the CPU tier's figure, + the first-order effect of forming F = l_F r_F^T in fp64 (the CPU tier
    takes F as given): |dF| <= gamma_S |l_F| |r_F|^T entry by entry, |d std_d| <= rms_m dF[d], |d mean_d| <= mean_m dF[d], and
    d pen = M / (S + M) ((1 - 1 / sig_w) d sig_w + 2 mu_w d mu_w)"""
    F = l_F @ r_F.T
    dF = PB.gamma(S, PB.U64) * (np.abs(l_F) @ np.abs(r_F).T)
    mF, sF, ml, sl = H.pen_rows(l_F, F)
    dsig = np.sqrt((dF ** 2).mean(1)).sum(); dmu = dF.mean(1).sum()
    pen = H.penalty(l_F, F)
    return 4 * H.MEASURED_PEN_ERR['pen'] * abs(pen) + M / (S + M) * (abs(1 - 1 / sF.sum()) * dsig + 2 * abs(mF.sum()) * dmu)


# (2, 70, 300): rows on either side of the 256-thread and 64-lane strides.  (64, 2, 70): K = 144, Kp = 256 -- the smallest geometry class
# at which the option lowrank_bwd's automatic rule fires (Dp >= 4 Sp and U fits in Phibar), so that fbar / grad_tail / lbar run
# their TZ / XU branches on the edge rows
@pytest.mark.parametrize('D,S,M', [(3, 2, 5), (2, 70, 300), (64, 2, 70)])
def test_penalty_edge_rows_on_the_device(D, S, M):
    X = synth.make_X(0x5CF6C010 + M, N, D)
    y = synth.normal(0x5CF6C011 + M, 0, N).reshape(-1, 1)
    eng = _engine(D, S, M)
    assert _lrb_rule(eng, S, -1) == (D == 64)
    eng.set_params(H.edge_params('sig_large', D, S, M)); eng.set_data(X, y)
    for case in H.EDGE_CASES:
        p = H.edge_params(case, D, S, M)
        l_F, r_F = H.edge_factors(case, D, S, M)
        eng.set_params(p)
        cost, grad, alpha, Li = eng.eval(want_grad=True)
        pen = eng.debug_read('scalars', (32,))[R_PEN]
        pen0 = float(KATS['pen/%d_%d_%d/%s' % (D, S, M, case)])
        allow = _pen_allowance(l_F, r_F, S, M)
        print('R_PEN (%d, %d, %d) %-9s %.15e  error %.2e  allowed %.2e' % (D, S, M, case, pen, abs(pen - pen0), allow), flush=True)
        assert abs(pen - pen0) <= allow, (case, pen, pen0)
        if M > 5:                                               # the penalty's part of the gradient, against the oracle
            c0, g0, a0, L0 = O.value_and_grad(X, y, p, S, M)
            assert abs(float(cost) - c0) < 1e-10 * max(1.0, abs(c0))
            assert np.linalg.norm(grad - g0) / np.linalg.norm(g0) < 1e-8
            PB.oracle_check((cost, grad, alpha, Li), X, y, p, S, M, 'f64', alpha_li=True, label='edge rows ' + case)
    eng.close()


# ---- fp32 mode along c --------------------------------------------------------------------------------------------------------------
def test_fp32_mode_along_c():
    """c does not touch cond(A): the c axis of the star under tests/parity.py's fp32 row, as test_ragged_and_degenerate_shapes calls it"""
    name = 'd3'
    D, S, M = SHAPES[name]
    X, y, params = (KATS['%s/%s' % (name, k)] for k in ('X', 'y', 'params'))
    eng = _engine(D, S, M, 'f32')
    eng.set_params(params); eng.set_data(X, y)
    cs = [abc[2] for abc in KATS[name + '/abc'] if abc[0] == -1.0 and abc[1] == 0.0]
    assert sorted(cs) == [-30.0, -20.0, -14.0, -10.0, -1.0, 10.0, 30.0]
    for c in cs:
        p = params.copy(); p[2] = c
        eng.set_params(p)
        res = eng.eval(want_grad=True)
        PB.oracle_check(res, X, y, p, S, M, 'f32', alpha_li=False, label='c = %g' % c)
    eng.close()


# ---- the posterior entry points at the ends of c ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('c', [-30.0, -20.0, 30.0])
def test_posterior_entry_points_at_the_ends_of_c(c, dtype):
    """predict against the oracle under test_ragged_and_degenerate_shapes' bound and, row by row, the sigma half of tests/parity.py's
    predict row (its mu half reads mu's error in units of sigma, which at c = -30 is 1e-7 of mu: there the row says nothing about
    kappa and no fp32 feature map can meet it), predict_cov with the noise on the diagonal under tests/test_gpu_predict_cov.py's
    bound, acquire's predictive sigma and UCB under tests/test_gpu_acquire.py's"""
    from tests.test_gpu_acquire import PARITY_BOUND
    from tests.test_gpu_predict_cov import BOUNDS
    D, S, M, T = 3, 1, 20, 301
    K = 2 * (S + M)
    seed = 0x5CF65000 + M
    params = synth.make_params(seed + 0x0202, D, S, M, abc=(-1.0, 0.0, c))
    rng = np.random.default_rng(seed)
    alpha = rng.standard_normal(K) / np.sqrt(K)
    Li = np.tril(rng.standard_normal((K, K))) / np.sqrt(K)
    Xs = synth.make_X(101, T, D)
    eng = _engine(D, S, M, dtype); eng.set_params(params)
    mu, sd = eng.predict(Xs, alpha, Li)
    mu0, sd0 = O.predict(Xs, alpha, Li, params, S, M)
    tol = 1e-8 if dtype == 'f64' else 2e-3                      # test_ragged_and_degenerate_shapes' bound on predict
    e_mu = np.linalg.norm(mu - mu0) / np.linalg.norm(mu0); e_sd = np.linalg.norm(sd - sd0) / np.linalg.norm(sd0)
    r_sd = float((np.abs(sd - sd0) / (PB.TOL[dtype]['eps'] * sd0)).max())          # tests/parity.py's predict row, its sigma half
    print('c = %g %s predict: mu %.2e std %.2e, worst row of std / allowed %.2e' % (c, dtype, e_mu, e_sd, r_sd))
    assert e_mu < tol and e_sd < tol and r_sd <= 1.0
    cov = eng.predict_cov(Xs, Li, noise=True)
    e = float(np.linalg.norm(cov - R.pred_cov(Xs, Li, params, S, M, noise=True)) / np.linalg.norm(cov))
    print('c = %g %s predict_cov %.2e' % (c, dtype, e))
    assert e < BOUNDS[dtype], e
    r = eng.acquire(Xs, alpha, Li, 'ucb', beta=2.5, noise=True, want=('acq', 'mu', 'sd'))
    assert np.array_equal(r['sd'], sd) and np.array_equal(r['mu'], mu.ravel())
    ref, _, _ = A.acquire('ucb', r['mu'], r['sd'], beta=2.5)
    assert A.kind_error('ucb', r['acq'], ref, r['mu'], r['sd'], 2.5) <= PARITY_BOUND['ucb']
    eng.close()


# ---- the degenerate row ---------------------------------------------------------------------------------------------------------------
def test_zero_std_rows_give_an_infinite_cost_and_the_context_recovers():
    """every row of l_F all-equal: the sum of their stds is 0 and the penalty +inf, as in the reference's formula (tests/test_hyper_ref.py
    pins it); the evaluation reports that cost, and the next valid one on the same context is the centre point's"""
    name = 'd3'
    D, S, M = SHAPES[name]
    K = 2 * (S + M)
    X, y, params = (KATS['%s/%s' % (name, k)] for k in ('X', 'y', 'params'))
    eng = _engine(D, S, M)
    eng.set_params(params); eng.set_data(X, y)
    p = params.copy()
    l_F = p[3:3 + D * S].reshape(D, S)
    l_F[:] = l_F[:, :1]
    with np.errstate(divide='ignore'):
        assert O._penalty(l_F, l_F @ p[3 + D * S:3 + D * S + M * S].reshape(M, S).T, S, M) == np.inf
    eng.set_params(p)
    with pytest.raises(FloatingPointError):
        eng.eval(want_grad=True)
    eng.nonfinite = 'return'
    cost = eng.eval(want_grad=True)[0]
    assert float(cost) == np.inf, cost
    eng.nonfinite = 'raise'
    eng.set_params(params)
    r = point_ratios(name, 0, eng.eval(want_grad=True), K)
    assert tuple(KATS[name + '/abc'][0]) == (-1.0, 0.0, -1.0)
    print('after the infinite cost, the centre: ' + PB.fmt(r))
    assert max(r.values()) <= 1.0, r
    eng.close()
