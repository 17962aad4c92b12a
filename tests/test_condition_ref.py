"""CPU tier of the posterior update (scfgp_condition): the numpy form (tests/condition_ref.py) on an oracle fit of the first N0 rows
against the oracle's own fit on all N0 + n rows, under the project's per-tile fp64 checks (tests/parity.py); its algebraic properties
(split, permutation, the predictive std never grows); and the C entry point's argument checks (no GPU needed)."""
import ctypes

import numpy as np
import pytest

from oracle import scfgp_oracle as O
from scfgp_amd import _lib
from tests import condition_ref as R
from tests import parity

# (D, S, M, N0, n): K = 128, 600, 2112, a small odd J, rank-S projection; n = 1, n < K, n > K, n not a multiple of anything
SHAPES = [(5, 4, 60, 1000, 300), (5, 4, 60, 1000, 1), (20, 20, 280, 3000, 700), (64, 32, 1024, 4000, 900), (3, 1, 20, 150, 400),
          (40, 4, 100, 2000, 129)]


def _fits(D, S, M, N0, n):
    params, X, y, Xs = R.problem(D, S, M, N0, n)
    _, a0, L0 = O.forward(X[:N0], y[:N0], params, S, M, gauss_hermite=False)
    _, a1, L1 = O.forward(X, y, params, S, M, gauss_hermite=False)
    return params, X, y, Xs, a0, L0, a1, L1


def _check(al, Li, a1, L1, Xs, params, S, M, label):
    mu1, sd1 = O.predict(Xs, a1, L1, params, S, M)
    mu, sd = O.predict(Xs, al, Li, params, S, M)
    r = dict(alpha=parity.alpha_ratio(al, a1, 'f64'), Li=parity.li_ratio(Li, L1, 'f64'), predict=parity.predict_ratio(mu, sd, mu1, sd1, 'f64'))
    print(label, parity.fmt(r))
    parity.check_alpha(al, a1, 'f64'); parity.check_li(Li, L1, 'f64'); parity.check_predict(mu, sd, mu1, sd1, 'f64')
    return r


@pytest.mark.parametrize('D,S,M,N0,n', SHAPES)
def test_update_equals_the_oracle_fit_on_all_rows(D, S, M, N0, n):
    params, X, y, Xs, a0, L0, a1, L1 = _fits(D, S, M, N0, n)
    al, Li = R.condition(X[N0:], y[N0:], a0, L0, params, S, M)
    assert al.shape == a1.shape and Li.shape == L1.shape and np.array_equal(Li, np.tril(Li))
    _check(al, Li, a1, L1, Xs, params, S, M, 'condition_ref %s' % ((D, S, M, N0, n),))
    # the check has teeth: the unconditioned factors miss even the looser fp32 bound in alpha
    assert parity.alpha_ratio(a0, a1, 'f32') > 1.0
    if n == 1:
        # one row moves Li by about the fp32 Li bound only, so the tile check above is weak evidence here: the MOVE itself must be right
        print('n = 1: the move of Li in units of the fp32 bound', parity.li_ratio(L0, L1, 'f32'))
        assert np.linalg.norm((Li - L0) - (L1 - L0)) <= 1e-6 * np.linalg.norm(L1 - L0)
    # entries above the diagonal of the incoming factor are not read
    junk = L0 + np.triu(np.full_like(L0, 7.0), 1)
    al2, Li2 = R.condition(X[N0:], y[N0:], a0, junk, params, S, M)
    assert np.array_equal(al2, al) and np.array_equal(Li2, Li)


@pytest.mark.parametrize('D,S,M,N0,n', [s for s in SHAPES if s[4] > 1])
def test_two_calls_on_a_split_and_a_permutation_equal_one_call(D, S, M, N0, n):
    params, X, y, Xs, a0, L0, a1, L1 = _fits(D, S, M, N0, n)
    h = N0 + n // 3
    am, Lm = R.condition(X[N0:h], y[N0:h], a0, L0, params, S, M)
    al, Li = R.condition(X[h:], y[h:], am, Lm, params, S, M)
    _check(al, Li, a1, L1, Xs, params, S, M, 'split %s' % ((D, S, M, N0, n),))
    perm = np.random.default_rng(M).permutation(n)
    al, Li = R.condition(X[N0:][perm], y[N0:][perm], a0, L0, params, S, M)
    _check(al, Li, a1, L1, Xs, params, S, M, 'permutation %s' % ((D, S, M, N0, n),))


@pytest.mark.parametrize('D,S,M,N0,n', SHAPES)
def test_conditioning_never_raises_the_predictive_std(D, S, M, N0, n):
    params, X, y, Xs, a0, L0, a1, L1 = _fits(D, S, M, N0, n)
    al, Li = R.condition(X[N0:], y[N0:], a0, L0, params, S, M)
    _, sd0 = O.predict(Xs, a0, L0, params, S, M)
    _, sd = O.predict(Xs, al, Li, params, S, M)
    assert np.all(sd <= sd0 * (1 + 1e-12))


def test_entry_point_declared_exported_and_checked_without_gpu():
    """scfgp_condition is in the header, the library and the binding table, and refuses bad arguments with a message before touching
    a device."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'scfgp_hip.h')).read(), flags=re.S)
    assert re.search(r'\bscfgp_condition\s*\(', header)
    assert 'scfgp_condition' in _lib.SIGNATURES
    lib = _lib.load()
    f = lib.scfgp_condition
    assert len(f.argtypes) == 9
    D, S, M = 3, 2, 5
    K = 2 * (S + M)
    Xn = np.zeros((4, D)); yn = np.zeros(4); al = np.zeros(K); Li = np.eye(K); ao = np.full(K, 3.0); Lo = np.full((K, K), 3.0)
    p = _lib.dptr
    assert f(None, p(Xn), p(yn), 4, p(al), p(Li), 0, p(ao), p(Lo)) == -1
    ctx = ctypes.c_void_p()
    lib.scfgp_create(ctypes.byref(ctx), D, S, M, 0, 0, None)        # fails on a GPU-less box but hands back its context
    assert ctx.value
    try:
        err = lambda: lib.scfgp_last_error(ctx)
        good = [p(Xn), p(yn), 4, p(al), p(Li), 0, p(ao), p(Lo)]
        for i in (0, 1, 3, 4, 6, 7):                               # every pointer
            args = list(good); args[i] = None
            assert f(ctx, *args) == -1
            assert b'bad arguments' in err()
        for mode in (-1, 2):
            args = list(good); args[5] = mode
            assert f(ctx, *args) == -1
            assert b'bad arguments' in err()
        for n in (0, -3):
            args = list(good); args[2] = n
            assert f(ctx, *args) == -1
            assert b'n must be at least 1' in err()
        args = list(good); args[5] = 1
        assert f(ctx, *args) == -1                                  # no X scaler registered
        assert b'scaler' in err()
        assert f(ctx, *good) == -1                                  # parameters not set
        assert b'parameters' in err()
        assert np.all(ao == 3.0) and np.all(Lo == 3.0)              # the outputs are untouched
    finally:
        lib.scfgp_destroy(ctx)
