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


def _agree(ds, scores, ds0, scores0):
    """replay_chol's arrays against replay's: d to 1e-12 of the row's start value (the two sum in different orders), the same rows
    eligible at every step"""
    if ds.shape != ds0.shape or scores.shape != scores0.shape or not np.array_equal(np.isfinite(scores), np.isfinite(scores0)):
        return False
    live = np.isfinite(scores0)
    tol = 1e-12 * np.broadcast_to(ds0[0], scores0.shape)
    return bool(np.all(np.abs(ds - ds0) <= 1e-12 * ds0[0])) and bool(np.all(np.abs(scores[live] - scores0[live]) <= tol[live]))


@pytest.mark.parametrize('case', R.CASES)
def test_cholesky_replay_equals_the_recurrence(case):
    D, S, M, N0, T, m = case
    if case in CASES:
        params, X0, y0, Xp, alpha, Li, C, ref = _setup(case)
        idx = ref['idx']
    else:                                                       # the headline K: no fit (it takes seconds), a synthetic factor
        params, Li, Xp = R.synthetic_problem(D, S, M, T)
        C = pred_cov_ref.factor(Xp, Li, params, S, M)
        idx = R.select(C, m)['idx']
    ds0, scores0 = R.replay(C, None, idx)
    ds, scores, dp = R.replay_chol(C, None, idx)
    worst = float((np.abs(ds - ds0) / ds0[0]).max())
    print('select ref %s: Cholesky replay against the recurrence, worst |d - d_rec| / d0 %.3g' % (case, worst))
    assert _agree(ds, scores, ds0, scores0)
    assert np.allclose(dp, ds0[np.arange(m), idx], rtol=1e-9, atol=0)
    # weights, a row of weight 0 among them
    w = 0.5 + np.random.default_rng(4).random(T); w[idx[1]] = 0.0
    idw = R.select(C, min(m, 10), w=w)['idx']
    assert _agree(*R.replay_chol(C, w, idw)[:2], *R.replay(C, w, idw))
    # the mutation: one pick swapped for its runner-up among the rows outside the sequence (every row is picked: for its successor)
    # must not pass as the same sequence
    j = m // 2
    swapped = idx.copy()
    if m < T:
        s = scores0[j].copy(); s[idx] = -np.inf
        swapped[j] = int(np.argmax(s))
    else:
        swapped[[j, j + 1]] = idx[[j + 1, j]]
    assert not _agree(*R.replay_chol(C, None, swapped)[:2], ds0, scores0)


@pytest.mark.parametrize('T,rpw', [(262144, 64), (262145, 128), (262144 + 69, 128), (524288, 128), (524289, 256), (1 << 20, 256)])
def test_edge_rows_sit_where_the_sweeps_index(T, rpw):
    """the inputs of tests/test_gpu_select_bounds.py: select.hip's rows per workgroup, and weighted rows at every edge of that tiling"""
    assert R.rows_per_group(T) == rpw and (T + rpw - 1) // rpw <= 4096
    rows = R.edge_rows(T); w = R.edge_weights(T)
    last = (T - 1) // rpw * rpw
    assert len(rows) <= 64 and len(set(rows.tolist())) == len(rows) and rows.min() == 0 and rows.max() == T - 1
    assert {last - 1, last, min(last + 1, T - 1), T - 2, rpw - 1, rpw, 32767, 32768} <= set(rows.tolist())
    assert np.array_equal(np.flatnonzero(w), rows) and len(set(w[rows].tolist())) == len(rows) and np.argmax(w) == T - 1


def test_synthetic_factor_is_dense_lower_triangular_and_well_conditioned():
    Li = R.synthetic_factor(300)
    assert np.array_equal(Li, np.tril(Li)) and np.count_nonzero(Li) == 300 * 301 // 2
    assert np.linalg.cond(Li) < 10.0
    params, L2, Xp = R.synthetic_problem(4, 2, 10, 50)
    assert L2.shape == (24, 24) and Xp.shape == (50, 4) and tuple(params[:3]) == R.ABC


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
