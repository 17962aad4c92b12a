"""CPU tier of scfgp_select_qei: the numpy restatement (tests/select_qei_ref.py) on its own terms -- the telescoping identity between the
gains and the two q-EI sums, gains that never increase, the prefix property, distinct picks with the all-zero tail, the (1 - 1/e) bound
against the exhaustive optimum, the two mutations, the agreement of score0 with the closed-form expected improvement within its
Monte-Carlo error, and the presence of the entry point in the built library and the binding table."""
import ctypes
import math

import numpy as np
import pytest

from oracle import scfgp_oracle as O
from scfgp_amd import _lib, synth
from tests import acquire_ref as A
from tests import sample_ref as R
from tests import select_qei_ref as Q

D, S, M = 3, 1, 20
K = 2 * (S + M)


def _model():
    params = synth.make_params(77, D, S, M, abc=(-1.0, 0.0, -1.0))
    rng = np.random.default_rng(78)
    alpha = rng.standard_normal(K) / np.sqrt(K)
    Li = np.tril(rng.standard_normal((K, K))) / np.sqrt(K)
    return params, alpha, Li


def _block(T, nsamp, seed, xseed=79):
    params, alpha, Li = _model()
    return R.samples(synth.make_X(xseed, T, D), alpha, Li, params, S, M, nsamp, seed)


def _median_best(F, minimize):
    return float(np.median(F.min(axis=0) if minimize else F.max(axis=0)))


# (F, m, best, xi, w, pending, minimize): some samples start above b and some below; a mask; pending rows; a best so far above every
# sample that every score is 0 from the first pick on
def _cases():
    F = _block(60, 33, 5)
    w = np.ones(60); w[::4] = 0.0
    P = _block(3, 33, 5, xseed=80)
    far = float(F.max()) + 10.0
    out = []
    for minimize in (False, True):
        best = _median_best(F, minimize)
        out += [(F, 9, best, 0.0, None, None, minimize), (F, 9, best, 0.05, w, None, minimize), (F, 9, best, 0.0, w, P, minimize),
                (F, 5, -far if minimize else far, 0.0, w, None, minimize)]
    return out


def _check_identity(fn):
    for F, m, best, xi, w, P, minimize in _cases():
        idx, gain, _, mstate, qei = fn(F, m, best, xi, w, P, minimize)
        total = float(np.sum(gain))
        scale = max(abs(qei[1]), abs(qei[0]), total)
        assert abs(total - (qei[1] - qei[0])) <= (m + F.shape[1]) * 2.0 ** -53 * scale, (total, qei)
        assert qei[1] == Q.batch_qei(F, idx, best, xi, minimize, P)
        assert qei[0] == (Q.batch_qei(P, range(P.shape[0]), best, xi, minimize) if P is not None else 0.0)


def _check_monotone(fn):
    for F, m, best, xi, w, P, minimize in _cases():
        gain = fn(F, m, best, xi, w, P, minimize)[1]
        assert np.all(gain[1:] <= gain[:-1]) and np.all(gain >= 0.0)


def _check_prefix(fn):
    for F, m, best, xi, w, P, minimize in _cases():
        full = fn(F, m, best, xi, w, P, minimize)
        part = fn(F, 3, best, xi, w, P, minimize)
        assert np.array_equal(part[0], full[0][:3]) and np.array_equal(part[1], full[1][:3]) and np.array_equal(part[2], full[2])


def _check_picks(fn):
    for F, m, best, xi, w, P, minimize in _cases():
        idx, gain = fn(F, m, best, xi, w, P, minimize)[:2]
        assert len(set(idx.tolist())) == m and idx.min() >= 0 and idx.max() < F.shape[0]
        if w is not None:
            assert np.all(w[idx] > 0)
        if np.all(gain == 0.0):                                     # the all-zero tail: the lowest eligible indices, in order
            rows = np.arange(F.shape[0]) if w is None else np.flatnonzero(w > 0)
            assert np.array_equal(idx, rows[:m])


CHECKS = (_check_identity, _check_monotone, _check_prefix, _check_picks)


@pytest.mark.parametrize('check', CHECKS)
def test_properties(check):
    check(Q.greedy)


def test_the_cases_cover_both_regimes():
    zero_tail = 0
    for F, m, best, xi, w, P, minimize in _cases():
        gain = Q.greedy(F, m, best, xi, w, P, minimize)[1]
        zero_tail += bool(np.all(gain == 0.0))
        if not np.all(gain == 0.0):
            assert gain[0] > 0.0 and np.count_nonzero(gain) >= 3
    assert zero_tail == 2


@pytest.mark.parametrize('mutation', ['forget_taken', 'update_before_gain'])
def test_mutations_are_caught(mutation):
    def mutant(F, m, best, xi, w, P, minimize):
        return Q.greedy(F, m, best, xi, w, P, minimize, **{mutation: True})
    caught = []
    for check in CHECKS:
        try:
            check(mutant)
        except AssertionError:
            caught.append(check.__name__)
    print(mutation, 'caught by', caught)
    assert caught


def test_greedy_against_exhaustive():
    T, m, nsamp = 10, 3, 32
    for seed in range(20):
        F = _block(T, nsamp, seed, xseed=100 + seed)
        for minimize in (False, True):
            best = _median_best(F, minimize)
            got = Q.greedy(F, m, best, minimize=minimize)
            opt = Q.exhaustive(F, m, best, minimize=minimize)
            assert got[4][1] == Q.batch_qei(F, got[0], best, minimize=minimize)
            assert opt > 0.0 and got[4][1] <= opt
            assert got[4][1] >= (1.0 - 1.0 / math.e) * opt, (seed, minimize, got[4][1], opt)


# score0 is a mean of nsamp independent draws of max(u - b, 0), u ~ N(sgn mu, sigma_f^2): its expectation is the closed-form EI of
# tests/acquire_ref.py with the latent sigma, and its standard error follows from E[max(u - b, 0)^2] = (sigma^2 + d^2) Phi(d / sigma) +
# sigma d phi(d / sigma), d = sgn mu - b.  6 s.e. at 64 rows: a false alarm has probability ~1e-7, and the seed is fixed.
@pytest.mark.parametrize('minimize', [False, True])
def test_score0_agrees_with_closed_form_ei(minimize):
    T, nsamp = 64, 1024
    params, alpha, Li = _model()
    Xs = synth.make_X(81, T, D)
    F = R.samples(Xs, alpha, Li, params, S, M, nsamp, 17)
    Phi = O.feature_map(Xs, params, D, S, M)
    mu = Phi @ alpha
    sd = A.sigma(R.kappa(params), np.sum((Phi @ np.tril(Li).T) ** 2, axis=1), False)
    sgn = -1.0 if minimize else 1.0
    best, xi = float(np.median(mu)), 0.01
    ei = A.acquire('ei', mu, sd, best=best, xi=xi, minimize=minimize)[0]
    d = sgn * mu - (sgn * best + xi)
    second = (sd ** 2 + d ** 2) * A.cdf(d / sd) + sd * d * A.pdf(d / sd)
    se = np.sqrt(np.maximum(second - ei ** 2, 0.0) / nsamp)
    score0 = Q.greedy(F, 1, best, xi, minimize=minimize)[2]
    z = np.abs(score0 - ei) / se
    print('largest deviation %.2f s.e.; EI from %.2e to %.2e' % (z.max(), ei.min(), ei.max()))
    assert np.all(np.abs(score0 - ei) <= 6.0 * se)
    assert np.median(z) > 0.05                                      # the bound is not vacuous: the two are different computations


def test_entry_point_is_exported_and_bound():
    assert 'scfgp_select_qei' in _lib.SIGNATURES
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, 'scfgp_select_qei')
    res, args = _lib.SIGNATURES['scfgp_select_qei']
    assert res is ctypes.c_int and len(args) == 20
