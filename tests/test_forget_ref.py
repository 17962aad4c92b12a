"""CPU tier of the posterior downdate (scfgp_forget): the numpy form (tests/forget_ref.py) on an oracle fit of all N0 + n rows against
the oracle's own fit on the first N0 rows, under the project's per-tile fp64 checks (tests/parity.py); the round trip with
condition_ref; agreement with loo_ref on consecutive blocks; the predictive std never shrinks; rows that were not in the fit; and the C
entry point's argument checks (no GPU needed)."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import scfgp_oracle as O
from scfgp_amd import _lib
from tests import condition_ref as CR
from tests import forget_ref as R
from tests import loo_ref
from tests import parity

# (D, S, M, N0, n): n rows are removed from a fit on N0 + n, N0 remain.  K = 128, 600, a small odd J, rank-S projection; n = 1, n < K,
# n > K, n not a multiple of anything, and most of the fit removed (1000 of 1300)
SHAPES = [(5, 4, 60, 1000, 300), (5, 4, 60, 1000, 1), (20, 20, 280, 3000, 700), (3, 1, 20, 150, 400), (40, 4, 100, 2000, 129),
          (5, 4, 60, 300, 1000)]


@functools.lru_cache(maxsize=None)
def _fits(D, S, M, N0, n):
    params, X, y, Xs = CR.problem(D, S, M, N0, n)
    _, a0, L0 = O.forward(X[:N0], y[:N0], params, S, M, gauss_hermite=False)
    _, a1, L1 = O.forward(X, y, params, S, M, gauss_hermite=False)
    return params, X, y, Xs, a0, L0, a1, L1


def _check(al, Li, a0, L0, Xs, params, S, M, label):
    mu0, sd0 = O.predict(Xs, a0, L0, params, S, M)
    mu, sd = O.predict(Xs, al, Li, params, S, M)
    r = dict(alpha=parity.alpha_ratio(al, a0, 'f64'), Li=parity.li_ratio(Li, L0, 'f64'), predict=parity.predict_ratio(mu, sd, mu0, sd0, 'f64'))
    print(label, parity.fmt(r))
    parity.check_alpha(al, a0, 'f64'); parity.check_li(Li, L0, 'f64'); parity.check_predict(mu, sd, mu0, sd0, 'f64')
    return r


@pytest.mark.parametrize('D,S,M,N0,n', SHAPES)
def test_downdate_equals_the_oracle_fit_on_the_remaining_rows(D, S, M, N0, n):
    params, X, y, Xs, a0, L0, a1, L1 = _fits(D, S, M, N0, n)
    out = R.forget(X[N0:], y[N0:], a1, L1, params, S, M)
    al, Li = out['alpha'], out['Li']
    assert al.shape == a0.shape and Li.shape == L0.shape and np.array_equal(Li, np.tril(Li))
    print('lam_min(S) %.3f  min M_ii^2 %.3f' % (out['lam_min'], out['stats'][5]))
    assert 0.0 < out['lam_min'] <= out['stats'][5] <= 1.0
    _check(al, Li, a0, L0, Xs, params, S, M, 'forget_ref %s' % ((D, S, M, N0, n),))
    # the check has teeth: the un-downdated factors miss even the looser fp32 bound in alpha
    assert parity.alpha_ratio(a1, a0, 'f32') > 1.0
    # the held-out predictions are the oracle's predict of the removed rows from the fit on the remaining ones
    mu0, sd0 = O.predict(X[N0:], a0, L0, params, S, M)
    parity.check_predict(out['mu'].reshape(-1, 1), out['std'], mu0, sd0, 'f64')
    # entries above the diagonal of the incoming factor are not read
    out2 = R.forget(X[N0:], y[N0:], a1, L1 + np.triu(np.full_like(L1, 7.0), 1), params, S, M)
    assert np.array_equal(out2['alpha'], al) and np.array_equal(out2['Li'], Li)


@pytest.mark.parametrize('D,S,M,N0,n', [SHAPES[0], SHAPES[1], SHAPES[3], SHAPES[5]])
def test_forget_undoes_condition(D, S, M, N0, n):
    params, X, y, Xs, a0, L0, a1, L1 = _fits(D, S, M, N0, n)
    ac, Lc = CR.condition(X[N0:], y[N0:], a0, L0, params, S, M)
    out = R.forget(X[N0:], y[N0:], ac, Lc, params, S, M)
    _check(out['alpha'], out['Li'], a0, L0, Xs, params, S, M, 'round trip %s' % ((D, S, M, N0, n),))


@pytest.mark.parametrize('D,S,M,N0,n', [SHAPES[0], SHAPES[2], SHAPES[3]])
def test_two_disjoint_sets_in_either_order_agree(D, S, M, N0, n):
    params, X, y, Xs, a0, L0, a1, L1 = _fits(D, S, M, N0, n)
    h = N0 + n // 3
    A, B = (X[N0:h], y[N0:h]), (X[h:], y[h:])
    res = []
    for first, second in ((A, B), (B, A)):
        o1 = R.forget(first[0], first[1], a1, L1, params, S, M)
        o2 = R.forget(second[0], second[1], o1['alpha'], o1['Li'], params, S, M)
        _check(o2['alpha'], o2['Li'], a0, L0, Xs, params, S, M, 'two sets %s' % ((D, S, M, N0, n),))
        res.append(o2)
    parity.check_alpha(res[0]['alpha'], res[1]['alpha'], 'f64'); parity.check_li(res[0]['Li'], res[1]['Li'], 'f64')


@pytest.mark.parametrize('block', [1, 7, 64])
def test_agrees_with_loo_ref_on_a_block_of_consecutive_rows(block):
    D, S, M, N0, n = SHAPES[2]
    params, X, y, Xs, a0, L0, a1, L1 = _fits(D, S, M, N0, n)
    i0 = 448                                                             # a multiple of every block size: the block is one of loo's
    ref = loo_ref.loo(X[:i0 + block], y[:i0 + block], a1, L1, params, S, M, block=block)
    out = R.forget(X[i0:i0 + block], y[i0:i0 + block], a1, L1, params, S, M)
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))))
    d = dict(mu=rel(out['mu'], ref['mu'][i0:]), std=rel(out['std'], ref['std'][i0:]), joint=rel(out['stats'][4], ref['joint'][-1]))
    print('block %d' % block, d)
    assert max(d.values()) <= 1e-9


@pytest.mark.parametrize('D,S,M,N0,n', SHAPES)
def test_removal_never_lowers_the_predictive_std(D, S, M, N0, n):
    params, X, y, Xs, a0, L0, a1, L1 = _fits(D, S, M, N0, n)
    out = R.forget(X[N0:], y[N0:], a1, L1, params, S, M)
    _, sd1 = O.predict(Xs, a1, L1, params, S, M)
    _, sd = O.predict(Xs, out['alpha'], out['Li'], params, S, M)
    assert np.all(sd >= sd1 * (1 - 1e-12))


def test_rows_that_were_not_in_the_fit_have_no_factor():
    D, S, M, N0, n = SHAPES[0]
    params, X, y, Xs, a0, L0, a1, L1 = _fits(D, S, M, N0, n)
    Xo, yo, k, h = R.tiled_row(X, y, a1, L1, params, S, M, i=3)
    assert k * h >= 2.0 and 0.0 < h < 1.0
    with pytest.raises(np.linalg.LinAlgError):
        R.forget(Xo, yo, a1, L1, params, S, M)
    R.forget(Xo[:1], yo[:1], a1, L1, params, S, M)                       # the row itself, once, is in the fit


def test_entry_point_declared_exported_and_checked_without_gpu():
    """scfgp_forget is in the header, the library and the binding table, and refuses bad arguments with a message before touching a
    device."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'scfgp_hip.h')).read(), flags=re.S)
    assert re.search(r'\bscfgp_forget\s*\(', header)
    assert 'scfgp_forget' in _lib.SIGNATURES
    lib = _lib.load()
    f = lib.scfgp_forget
    assert len(f.argtypes) == 12
    D, S, M = 3, 2, 5
    K = 2 * (S + M)
    Xo = np.zeros((4, D)); yo = np.zeros(4); al = np.zeros(K); Li = np.eye(K)
    outs = [np.full(K, 3.0), np.full((K, K), 3.0), np.full(4, 3.0), np.full(4, 3.0), np.full(8, 3.0)]
    p = _lib.dptr
    good = [p(Xo), p(yo), 4, p(al), p(Li), 0] + [p(o) for o in outs]
    assert f(None, *good) == -1
    ctx = ctypes.c_void_p()
    lib.scfgp_create(ctypes.byref(ctx), D, S, M, 0, 0, None)        # fails on a GPU-less box but hands back its context
    assert ctx.value
    try:
        err = lambda: lib.scfgp_last_error(ctx)

        def refused(text, **change):
            args = list(good)
            for i, v in change.items():
                args[int(i[1:])] = v
            assert f(ctx, *args) == -1
            assert text in err(), err()
        for i in (0, 1, 3, 4):                                         # every input pointer
            refused(b'bad arguments', **{'a%d' % i: None})
        for mode in (-1, 2):
            refused(b'bad arguments', a5=mode)
        refused(b'alpha_out and Li_out go together', a6=None)
        refused(b'alpha_out and Li_out go together', a7=None)
        refused(b'mu and std go together', a8=None)
        refused(b'mu and std go together', a9=None)
        refused(b'stats need mu and std', a8=None, a9=None)
        refused(b'no output asked for', a6=None, a7=None, a8=None, a9=None, a10=None)
        for n in (0, -3):
            refused(b'n must be at least 1', a2=n)
        refused(b'scaler', a5=1)                                       # no X scaler registered
        refused(b'parameters')                                         # parameters not set
        assert all(np.all(o == 3.0) for o in outs)                     # the outputs are untouched
    finally:
        lib.scfgp_destroy(ctx)
