"""CPU tier of the greedy choice by integrated variance reduction (scfgp_select_iv): tests/select_iv_ref.py's recurrences against the
oracle.  The score of EVERY eligible row times kappa is the drop of the oracle's sum_r omega_r sigma_r^2 when that row joins the refit;
the integrated variance after the picks is the oracle's refit on the old rows plus the picks; a after the picks is c^T P Q P c formed
directly; prefixes; the criterion is not scfgp_select's; and dropping the (q / 2) u_j term is caught."""
import functools

import numpy as np
import pytest

from oracle import scfgp_oracle as O
from tests import parity, pred_cov_ref
from tests import select_iv_ref as V
from tests import select_ref as R

EPS = parity.TOL['f64']['eps']
REFS = ('pool', 'subset')


@functools.lru_cache(maxsize=None)
def _fit(case):
    D, S, M, N0, T, m = case
    params, X0, y0, Xp = R.problem(case)
    _, alpha, Li = O.forward(X0, y0, params, S, M, gauss_hermite=False)
    return params, X0, y0, Xp, alpha, Li, pred_cov_ref.factor(Xp, Li, params, S, M)


def reference_set(case, which):
    """(rows of the pool, weights or None) of the issue's two reference sets"""
    T = case[4]
    return (np.arange(T), None) if which == 'pool' else V.subset_reference(T)


@functools.lru_cache(maxsize=None)
def _setup(case, which):
    params, X0, y0, Xp, alpha, Li, C = _fit(case)
    rows, om = reference_set(case, which)
    Q = V.gram(C[rows], om)
    return Q, rows, om, V.select(C, Q, case[5], kap=R.kappa(params))


def integrated_variance(case, which, picks):
    """the oracle's sum_r omega_r sigma_r^2 over the reference rows from its own refit on the old rows plus the rows `picks` of the pool
    (zero targets), and the sum of the project's predictive bound over the same rows"""
    D, S, M, N0, T, m = case
    params, X0, y0, Xp = _fit(case)[:4]
    rows, om = reference_set(case, which)
    om = np.ones(len(rows)) if om is None else om
    picks = list(picks)
    Xa = np.vstack([X0, Xp[picks]]) if picks else X0
    ya = np.vstack([y0, np.zeros((len(picks), 1))])
    _, a2, L2 = O.forward(Xa, ya, params, S, M, gauss_hermite=False)
    sd = O.predict(Xp[rows], a2, L2, params, S, M)[1].ravel()
    # |d sigma| <= eps sigma  =>  |d sigma^2| <= (2 + eps) eps sigma^2
    return float(om @ sd ** 2), float(om @ ((2.0 + EPS) * EPS * sd ** 2)), float(om.sum())


def test_every_score_is_the_drop_of_the_oracles_integrated_variance(half_q=True):
    case = R.CASES[1]
    params, X0, y0, Xp, alpha, Li, C = _fit(case)
    kap = R.kappa(params)
    Q, rows, om, ref = _setup(case, 'pool')
    if not half_q:
        ref = V.select(C, Q, case[5], kap=kap, half_q=False)
    worst = 0.0
    for step in (0, 5):
        picks = ref['idx'][:step].tolist()
        _, _, scores, _ = V.replay(C, Q, None, ref['idx'][:step + 1]) if half_q else (None, None, _mutant_scores(C, Q, ref, step), None)
        before, bound0, _ = integrated_variance(case, 'pool', picks)
        eligible = np.flatnonzero(np.isfinite(scores[step]))
        assert len(eligible) == case[4] - step
        for i in eligible:
            after, bound1, _ = integrated_variance(case, 'pool', picks + [int(i)])
            err = abs(kap * scores[step][i] - (before - after))
            worst = max(worst, err / (bound0 + bound1))
    print('select_iv ref %s: worst score against the refit drop, ratio to the f64 bound %.3g' % (case, worst))
    assert worst <= 1.0


def _mutant_scores(C, Q, ref, step):
    """the scores before step `step` of the recurrence without its (q / 2) u_j term, along the mutant's own picks"""
    T, K = C.shape
    a = np.einsum('ik,ik->i', C @ Q, C); d = np.sum(C * C, axis=1)
    U = np.empty((0, K)); taken = np.zeros(T, bool)
    out = []
    for p in ref['idx'][:step + 1]:
        out.append(V._scores(np.ones(T), a, d, taken))
        u, dp, q, a, d = V._step(C, Q, U, int(p), a, d, half_q=False)
        U = np.vstack([U, u]); taken[int(p)] = True
    return out


def test_dropping_the_half_q_term_fails_the_refit_comparison():
    with pytest.raises(AssertionError):
        test_every_score_is_the_drop_of_the_oracles_integrated_variance(half_q=False)


@pytest.mark.parametrize('which', REFS)
@pytest.mark.parametrize('case', R.CASES)
def test_integrated_variance_equals_the_oracles_refit(case, which):
    params = _fit(case)[0]
    kap = R.kappa(params)
    Q, rows, om, ref = _setup(case, which)
    for k, picks in ((0, []), (1, ref['idx'].tolist())):
        total, bound, osum = integrated_variance(case, which, picks)
        err = abs(ref['ivar'][k] - (total - kap * osum))
        print('select_iv ref %s %s: ivar[%d] %.6g, against the refit: ratio to the f64 bound %.3g' % (case, which, k, ref['ivar'][k], err / bound))
        assert err <= bound
    assert np.all(ref['red'] > 0) and ref['ivar'][1] < ref['ivar'][0]
    assert abs(ref['ivar'][0] - ref['red'].sum() - ref['ivar'][1]) <= 1e-12 * ref['ivar'][0]
    # q_j is the winning score: a_p / (1 + d_p) at the moment of the pick
    As, Ds, scores, qs = V.replay(_fit(case)[6], Q, None, ref['idx'])
    m = case[5]
    assert np.allclose(scores[np.arange(m), ref['idx']], qs, rtol=1e-9, atol=1e-12 * qs.max())


@pytest.mark.parametrize('which', REFS)
@pytest.mark.parametrize('case', R.CASES)
def test_a_equals_the_quadratic_form_formed_directly(case, which):
    C = _fit(case)[6]
    Q, rows, om, ref = _setup(case, which)
    P = np.eye(C.shape[1]) - ref['U'].T @ ref['U']
    CP = C @ P
    direct = np.einsum('ik,ik->i', CP @ Q, CP)
    err = float(np.abs(ref['a'] - direct).max() / ref['a0'].max())
    print('select_iv ref %s %s: a after %d picks against c^T P Q P c: %.3g of max a' % (case, which, case[5], err))
    assert err <= 1e-12
    assert np.allclose(ref['d'], np.sum(CP * C, axis=1), rtol=0, atol=1e-12 * ref['d0'].max())


@pytest.mark.parametrize('case', R.CASES[:3])
def test_prefix_property_and_replay(case):
    params, X0, y0, Xp, alpha, Li, C = _fit(case)
    Q, rows, om, ref = _setup(case, 'subset')
    short = V.select(C, Q, 7, kap=R.kappa(params))
    for k in ('idx', 'red', 'var', 'gap'):
        assert np.array_equal(short[k], ref[k][:7])
    As, Ds, scores, qs = V.replay(C, Q, None, ref['idx'])
    assert np.array_equal(As[-1], ref['a']) and np.array_equal(Ds[-1], ref['d'])
    assert np.array_equal(np.argmax(scores, axis=1), ref['idx'])
    assert np.array_equal(R.kappa(params) * qs, ref['red'])


@pytest.mark.parametrize('case', R.CASES)
def test_the_criterion_is_not_the_maximum_information_one(case):
    params, X0, y0, Xp, alpha, Li, C = _fit(case)
    m = case[5]
    info = R.select(C, m)['idx']
    ident = V.select(C, np.eye(C.shape[1]), m)['idx']
    assert ident[0] == info[0]                                   # a = d at the start: d / (1 + d) grows with d
    assert not np.array_equal(ident, info)
    pool = _setup(case, 'pool')[3]['idx']
    assert not np.array_equal(pool[:2], info[:2])


@pytest.mark.parametrize('which', REFS)
@pytest.mark.parametrize('case', R.CASES)
def test_gaps_the_gpu_tier_relies_on(case, which):
    ref = _setup(case, which)[3]
    print('select_iv ref %s %s: smallest relative gap between the best and the second-best score %.3g' % (case, which, ref['gap'].min()))
    assert ref['gap'].min() > 1e-8


def test_weights():
    case = R.CASES[0]
    params, X0, y0, Xp, alpha, Li, C = _fit(case)
    Q, rows, om, ref = _setup(case, 'pool')
    T = case[4]
    w = np.ones(T); w[ref['idx'][:5]] = 0.0                     # the five best rows are not for sale
    out = V.select(C, Q, 10, w=w)
    assert not set(out['idx'].tolist()) & set(ref['idx'][:5].tolist())
    twice = V.select(C, Q, 10, w=2 * w)
    assert np.array_equal(twice['idx'], out['idx']) and np.array_equal(twice['red'], out['red'])
    # doubling the reference weights doubles every reduction and moves no pick
    dbl = V.select(C, 2.0 * Q, 10)
    assert np.array_equal(dbl['idx'], ref['idx'][:10]) and np.allclose(dbl['red'], 2.0 * ref['red'][:10] / R.kappa(params), rtol=1e-12)
    w3 = np.zeros(T); w3[[3, 77, 500]] = 1.0
    assert sorted(V.select(C, Q, 3, w=w3)['idx'].tolist()) == [3, 77, 500]
    with pytest.raises(AssertionError):
        V.select(C, Q, 4, w=w3)
