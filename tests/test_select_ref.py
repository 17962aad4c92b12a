"""CPU tier of the greedy selection (scfgp_select): tests/select_ref.py's three lines against the oracle.  The variance after the picks
equals the oracle's predictive std from its own refit on the old rows plus the picked rows (whatever the targets), directly and through
tests/condition_ref.py; the gains add up to the batch's log-determinant; the greedy batch beats random ones; prefixes; weights."""
import functools

import numpy as np
import pytest

from oracle import scfgp_oracle as O
from tests import condition_ref, parity, pred_cov_ref
from tests import select_ref as R

CASES = R.CASES[:3]                                             # the headline K is the GPU tier's (one oracle fit at K = 2112 takes seconds)


@functools.lru_cache(maxsize=None)
def _setup(case):
    D, S, M, N0, T, m = case
    params, X0, y0, Xp = R.problem(case)
    _, alpha, Li = O.forward(X0, y0, params, S, M, gauss_hermite=False)
    C = pred_cov_ref.factor(Xp, Li, params, S, M)
    return params, X0, y0, Xp, alpha, Li, C, R.select(C, m, kap=R.kappa(params))


@pytest.mark.parametrize('case', CASES)
def test_std_after_equals_the_oracles_refit(case):
    D, S, M, N0, T, m = case
    params, X0, y0, Xp, alpha, Li, C, ref = _setup(case)
    assert len(set(ref['idx'].tolist())) == m and np.all(np.isfinite(ref['std_after'])) and np.all(ref['d'] >= 0)
    rng = np.random.default_rng(3)
    for targets in (np.zeros((m, 1)), rng.standard_normal((m, 1))):          # the variance does not depend on the observed values
        Xa = np.vstack([X0, Xp[ref['idx']]]); ya = np.vstack([y0, targets])
        _, a2, L2 = O.forward(Xa, ya, params, S, M, gauss_hermite=False)
        mu0, sd0 = O.predict(Xp, a2, L2, params, S, M)
        r = parity.check_predict(mu0, ref['std_after'], mu0, sd0, 'f64')
        print('select ref %s: std_after against the refit, ratio to the f64 bound %.3g' % (case, r))
    # the same through the K x K update
    a3, L3 = condition_ref.condition(Xp[ref['idx']], np.zeros(m), alpha, Li, params, S, M)
    mu1, sd1 = O.predict(Xp, a3, L3, params, S, M)
    parity.check_predict(mu1, ref['std_after'], mu1, sd1, 'f64')
    # var[j] is kappa d_p at the moment of the pick; the first one is predict's own variance without the noise
    _, sd_before = O.predict(Xp, alpha, Li, params, S, M)
    kap = R.kappa(params)
    assert abs(ref['var'][0] - (np.max(sd_before) ** 2 - kap)) <= 1e-9 * kap * (1 + ref['var'][0] / kap)
    assert ref['idx'][0] == int(np.argmax(sd_before))


@pytest.mark.parametrize('case', CASES)
def test_gains_add_up_to_the_log_determinant(case):
    D, S, M, N0, T, m = case
    params, X0, y0, Xp, alpha, Li, C, ref = _setup(case)
    Cs = C[ref['idx']]
    _, logdet = np.linalg.slogdet(np.eye(m) + Cs @ Cs.T)
    assert abs(np.sum(ref['gain']) - 0.5 * logdet) <= 1e-9 * 0.5 * logdet
    # marginal gains of a submodular function never grow
    assert np.all(np.diff(ref['gain']) <= 1e-12 * ref['gain'][:-1])


@pytest.mark.parametrize('case', [CASES[0], CASES[2]])
def test_greedy_beats_random_subsets(case):
    D, S, M, N0, T, m = case
    params, X0, y0, Xp, alpha, Li, C, ref = _setup(case)
    rng = np.random.default_rng(11)
    best = np.sum(ref['gain'])
    for _ in range(20):
        Cs = C[rng.choice(T, size=m, replace=False)]
        assert best >= 0.5 * np.linalg.slogdet(np.eye(m) + Cs @ Cs.T)[1]


@pytest.mark.parametrize('case', CASES)
def test_prefix_property_and_replay(case):
    D, S, M, N0, T, m = case
    params, X0, y0, Xp, alpha, Li, C, ref = _setup(case)
    short = R.select(C, 7, kap=R.kappa(params))
    for k in ('idx', 'var', 'gain', 'gap'):
        assert np.array_equal(short[k], ref[k][:7])
    ds, scores = R.replay(C, None, ref['idx'])
    assert ds.shape == (m + 1, T) and np.array_equal(ds[-1], ref['d'])
    assert np.array_equal(np.argmax(scores, axis=1), ref['idx'])
    assert np.allclose(R.kappa(params) * ds[np.arange(m), ref['idx']], ref['var'], rtol=1e-9, atol=0)
    # the gaps the GPU tier relies on
    print('select ref %s: smallest relative gap between the best and the second-best score %.3g' % (case, ref['gap'].min()))
    assert ref['gap'].min() > 1e-8


def test_weights():
    case = CASES[0]
    D, S, M, N0, T, m = case
    params, X0, y0, Xp, alpha, Li, C, ref = _setup(case)
    w = np.ones(T); w[ref['idx'][:5]] = 0.0                     # the five best rows are not for sale
    out = R.select(C, 10, w=w, kap=R.kappa(params))
    assert not set(out['idx'].tolist()) & set(ref['idx'][:5].tolist())
    assert out['idx'][0] == ref['idx'][5] or out['var'][0] <= ref['var'][0]
    # a weight scales the score, not the variance: doubling every weight changes nothing
    twice = R.select(C, 10, w=2 * w, kap=R.kappa(params))
    assert np.array_equal(twice['idx'], out['idx']) and np.array_equal(twice['var'], out['var'])
    # a heavy row goes first
    w2 = np.ones(T); heavy = int(np.argmin(np.sum(C * C, axis=1))); w2[heavy] = 1e6
    assert R.select(C, 3, w=w2, kap=R.kappa(params))['idx'][0] == heavy
    # exactly m eligible rows: all of them, and one more is refused
    w3 = np.zeros(T); w3[[3, 77, 500]] = 1.0
    assert sorted(R.select(C, 3, w=w3)['idx'].tolist()) == [3, 77, 500]
    with pytest.raises(AssertionError):
        R.select(C, 4, w=w3)


def _long_reference(case):
    D, S, M, N0, T, m = case
    params, X0, y0, Xp = R.problem(case)
    _, alpha, Li = O.forward(X0, y0, params, S, M, gauss_hermite=False)
    C = pred_cov_ref.factor(Xp, Li, params, S, M)
    w = R.long_weights(T)
    return w, R.select(C, m, w=w, kap=R.kappa(params))


def test_long_case_picks_from_both_sides_of_the_chunk_boundary():
    w, ref = _long_reference(R.LONG)
    assert np.all(w[ref['idx']] > 0) and ref['idx'].min() < 32768 <= ref['idx'].max()
    assert ref['gap'].min() > 1e-8


def test_three_chunk_case_picks_from_every_chunk():
    w, ref = _long_reference(R.LONG3)
    idx = ref['idx']
    print('select ref %s: picks %s, smallest gap %.3g' % (R.LONG3, idx.tolist(), ref['gap'].min()))
    assert np.all(w[idx] > 0) and idx.min() < 32768 and np.any((idx >= 32768) & (idx < 65536)) and idx.max() >= 65536
    assert ref['gap'].min() > 1e-8
