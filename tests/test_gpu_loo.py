"""GPU tier of the leave-block-out predictions (scfgp_loo).  The device is fed the ORACLE's fit on all rows, so only its own error
shows; every row is judged against the oracle refitted without the row's block (tests/loo_ref.py: refit) or, where that would take
thousands of refits, against loo_ref's fp64 form, which tests/test_loo_ref.py ties to the refits.  fp64 under the project's
predictive bound (tests/parity.py: TOL, unchanged); fp32 per row under TOL['f32']['eps'] sigma0 / (1 - lambda_max(H_I)): the
first-order amplification of a perturbation of H through (I - H)^-1.  Then: chunks, stats, resident rows, modes, errors, facade."""
import functools

import numpy as np
import pytest

from oracle import scfgp_oracle as O
from scfgp_amd import synth
from scfgp_amd.scaler import Scaler
from tests import loo_ref as R
from tests import parity

pytestmark = pytest.mark.gpu

# the table of tests/loo_ref.py and one shape at the headline K (its reference is loo_ref, not 24 refits at K = 2112)
BIG = ((64, 32, 1024, 1500, 64), (-1.0, 0.0, -1.0))
CASES = R.CASES + [BIG]
EPS = {'f64': parity.TOL['f64']['eps'], 'f32': parity.TOL['f32']['eps']}


@functools.lru_cache(maxsize=None)
def _fit(shape, abc):
    D, S, M, N, block = shape
    params, X, y = R.problem(D, S, M, N, abc)
    _, alpha, Li = O.forward(X, y, params, S, M, gauss_hermite=False)
    return params, X, y, alpha, Li


@functools.lru_cache(maxsize=None)
def _ref(shape, abc):
    D, S, M, N, block = shape
    params, X, y, alpha, Li = _fit(shape, abc)
    ref = R.loo(X, y, alpha, Li, params, S, M, block)
    mu0, sd0 = (ref['mu'], ref['std']) if (shape, abc) == BIG else R.refit(X, y, params, S, M, block)
    return ref, mu0, sd0


def _engine(D, S, M, dtype, params):
    from scfgp_amd.engine import HipEngine
    eng = HipEngine(D, S, M, dtype=dtype); eng.set_params(params)
    return eng


def _ratio32(mu, sd, mu0, sd0, lmax_rows):
    """worst over rows of max(|D mu|, |D sigma|) / (eps32 sigma0 / (1 - lambda_max of the row's block))"""
    d = np.maximum(np.abs(np.ravel(mu) - mu0), np.abs(np.ravel(sd) - sd0))
    return float((d * (1.0 - lmax_rows) / (EPS['f32'] * sd0)).max())


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('shape,abc', CASES)
def test_parity_with_refits_every_row(shape, abc, dtype):
    D, S, M, N, block = shape
    params, X, y, alpha, Li = _fit(shape, abc)
    ref, mu0, sd0 = _ref(shape, abc)
    eng = _engine(D, S, M, dtype, params)
    mu, sd, lev, st = eng.loo(X, y, alpha, Li, block=block)
    eng.close()
    assert mu.shape == (N, 1) and sd.shape == (N,) and lev.shape == (N,) and st['n'] == N and st['blocks'] == -(-N // block)
    lm = R.row_lmax(ref, N, block)
    r64 = parity.predict_ratio(mu, sd, mu0, sd0, 'f64')
    r32 = _ratio32(mu, sd, mu0, sd0, lm)
    print('loo parity %s abc %s %s: ratio to the f64 bound %.3g, to the f32 bound %.3g, lev err %.3g, lambda_max %.3g' %
          (shape, abc, dtype, r64, r32, np.abs(lev - ref['lev']).max(), ref['lmax'].max()))
    if dtype == 'f64':
        parity.check_predict(mu, sd, mu0, sd0, 'f64')
    else:
        assert r32 <= 1.0, ('held-out row outside its fp32 bound', shape, abc, r32)
    assert np.all(np.abs(lev - ref['lev']) <= (1e-9 if dtype == 'f64' else 1e-5) * np.maximum(ref['lev'], 1e-3))
    # the check has teeth: the in-sample prediction misses the fp32 bound by far
    mu_in, sd_in = O.predict(X, alpha, Li, params, S, M)
    assert _ratio32(mu_in, sd_in, mu0, sd0, lm) > 1.0


@functools.lru_cache(maxsize=None)
def _long():
    D, S, M, n, block = 5, 4, 60, 32768 + 300, 7
    params, X, y = R.problem(D, S, M, n + 4, (-1.0, 0.0, -1.0))
    _, alpha, Li = O.forward(X, y, params, S, M, gauss_hermite=False)
    return (D, S, M, n, block), params, X, y, alpha, Li


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_chunk_boundary_lands_on_a_block_boundary(dtype):
    """7 does not divide 32768: the first chunk holds 4681 blocks = 32767 rows.  n = 32768 + 300 is itself a multiple of 7, so the
    ragged last block of 4 rows comes from a second call on 4 more rows of the same fit."""
    (D, S, M, n, block), params, X, y, alpha, Li = _long()
    eng = _engine(D, S, M, dtype, params)
    mu, sd, lev, st = eng.loo(X[:n], y[:n], alpha, Li, block=block)
    lo, hi = 7 * 4680, 7 * 4690                                       # blocks 4680 .. 4689 around row 32768
    assert lo < 32767 < 32768 < hi and st['blocks'] == n // 7
    ref = R.loo(X[lo:hi], y[lo:hi], alpha, Li, params, S, M, block)
    lm = R.row_lmax(ref, hi - lo, block)
    r = (parity.predict_ratio(mu[lo:hi], sd[lo:hi], ref['mu'], ref['std'], 'f64') if dtype == 'f64' else
         _ratio32(mu[lo:hi], sd[lo:hi], ref['mu'], ref['std'], lm))
    print('chunk crossing %s: ratio %.3g' % (dtype, r))
    assert r <= 1.0
    mu2, sd2, lev2, _ = eng.loo(X[lo:hi], y[lo:hi], alpha, Li, block=block)
    assert np.array_equal(mu2, mu[lo:hi]) and np.array_equal(sd2, sd[lo:hi]) and np.array_equal(lev2, lev[lo:hi])
    # ragged last block: 33072 = 7 x 4724 + 4
    mu3, sd3, lev3, st3 = eng.loo(X, y, alpha, Li, block=block)
    assert st3['blocks'] == 4725 and st3['n'] == n + 4
    assert np.array_equal(mu3[:n], mu) and np.array_equal(sd3[:n], sd) and np.array_equal(lev3[:n], lev)
    ref3 = R.loo(X[n:], y[n:], alpha, Li, params, S, M, block)        # the 4 rows as one block
    r3 = (parity.predict_ratio(mu3[n:], sd3[n:], ref3['mu'], ref3['std'], 'f64') if dtype == 'f64' else
          _ratio32(mu3[n:], sd3[n:], ref3['mu'], ref3['std'], R.row_lmax(ref3, 4, block)))
    print('ragged last block %s: ratio %.3g' % (dtype, r3))
    assert r3 <= 1.0
    eng.close()


@functools.lru_cache(maxsize=None)
def _long3():
    D, S, M, n, block = 5, 4, 60, 65536 + 300, 7
    params, X, y = R.problem(D, S, M, n, (-1.0, 0.0, -1.0))
    _, alpha, Li = O.forward(X, y, params, S, M, gauss_hermite=False)
    return (D, S, M, n, block), params, X, y, alpha, Li


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_third_chunk_starts_on_a_block_boundary(dtype):
    """three chunks of 32767 rows: the third one reuses the first one's upload half and output half, and starts at row 65534 = 7 x 9362.
    65836 = 7 x 9405 + 1: the ragged last block is one row."""
    (D, S, M, n, block), params, X, y, alpha, Li = _long3()
    eng = _engine(D, S, M, dtype, params)
    mu, sd, lev, st = eng.loo(X, y, alpha, Li, block=block)
    lo, hi = 7 * 9360, 7 * 9370                                       # blocks 9360 .. 9369 around row 65534
    assert lo < 65534 < hi and st['blocks'] == 9406 and st['n'] == n
    ref = R.loo(X[lo:hi], y[lo:hi], alpha, Li, params, S, M, block)
    lm = R.row_lmax(ref, hi - lo, block)
    r = (parity.predict_ratio(mu[lo:hi], sd[lo:hi], ref['mu'], ref['std'], 'f64') if dtype == 'f64' else
         _ratio32(mu[lo:hi], sd[lo:hi], ref['mu'], ref['std'], lm))
    print('third chunk %s: ratio %.3g' % (dtype, r))
    assert r <= 1.0
    mu2, sd2, lev2, _ = eng.loo(X[lo:hi], y[lo:hi], alpha, Li, block=block)
    assert np.array_equal(mu2, mu[lo:hi]) and np.array_equal(sd2, sd[lo:hi]) and np.array_equal(lev2, lev[lo:hi])
    eng.close()


def _host_stats(mu, sd, lev, y):
    e = np.ravel(y) - np.ravel(mu)
    var = sd * sd
    marg = -0.5 * (e * e / var + np.log(2 * np.pi * var))
    return [(np.sum(e * e), np.sum(e * e)), (np.sum(np.abs(e)), np.sum(np.abs(e))), (np.sum(marg), np.sum(np.abs(marg)))]


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('shape,abc', [R.CASES[0], R.CASES[1], R.CASES[4], BIG])
def test_stats(shape, abc, dtype):
    D, S, M, N, block = shape
    params, X, y, alpha, Li = _fit(shape, abc)
    ref, _, _ = _ref(shape, abc)
    eng = _engine(D, S, M, dtype, params)
    mu, sd, lev, st = eng.loo(X, y, alpha, Li, block=block)
    again = eng.loo(X, y, alpha, Li, block=block)
    eng.close()
    assert np.array_equal(again[0], mu) and np.array_equal(again[1], sd) and np.array_equal(again[2], lev) and again[3] == st
    tol = 4 * parity.bound64(N)
    for key, (val, scale) in zip(('sum_e2', 'sum_abs_e', 'sum_log_marginal'), _host_stats(mu, sd, lev, y)):
        print('stats %s %s %s: device %.17g host %.17g, difference / abs-sum %.3g (bound %.3g)' %
              (shape, dtype, key, st[key], val, abs(st[key] - val) / scale, tol))
        assert abs(st[key] - val) <= tol * scale
    assert st['max_leverage'] == lev.max()
    if block == 1:
        assert st['sum_log_joint'] == st['sum_log_marginal']              # bit for bit
    else:
        lam = ref['lmax'].max()
        err = abs(st['sum_log_joint'] - ref['stats'][4]) / np.sum(np.abs(ref['joint']))
        print('stats %s %s sum_log_joint: %.17g against %.17g, error / abs-sum %.3g, bound %.3g' %
              (shape, dtype, st['sum_log_joint'], ref['stats'][4], err, EPS[dtype] / (1 - lam)))
        assert err <= EPS[dtype] / (1 - lam)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_resident_rows(dtype):
    from scfgp_amd.engine import HipEngine
    D, S, M, N = 20, 20, 280, 1500
    params = synth.make_params(7, D, S, M, abc=(-1.0, 0.0, -1.0))
    X = synth.make_X(7, N, D)
    y = np.sin(3 * X[:, :1]) + 0.1 * synth.normal(10, 0, N)[:, None]
    eng = HipEngine(D, S, M, dtype=dtype); eng.set_params(params); eng.set_data(X, y)
    c0, g0, a0, L0 = eng.eval(want_grad=True)
    c0, g0, a0, L0 = float(c0), g0.copy(), a0.copy(), L0.copy()
    for block in (1, 16):
        res = eng.loo(None, None, a0, L0, block=block)
        exp = eng.loo(X, y, a0, L0, block=block)
        for u, v in zip(res[:3], exp[:3]):
            assert np.array_equal(u, v)
        assert res[3] == exp[3] and res[3]['n'] == N
    c1, g1, a1, L1 = eng.eval(want_grad=True)
    assert float(c1) == c0 and np.array_equal(g1, g0) and np.array_equal(a1, a0) and np.array_equal(L1, L0)
    # a minibatch leaves a gathered working set behind: loo reads the stored rows, not that
    idx = np.arange(0, N, 3)
    eng.eval_rows(idx, want_grad=True)
    res = eng.loo(None, None, a0, L0, block=16)
    for u, v in zip(res[:3], exp[:3]):
        assert np.array_equal(u, v)
    c2, g2, a2, L2 = eng.eval(want_grad=True)
    assert float(c2) == c0 and np.array_equal(g2, g0) and np.array_equal(a2, a0) and np.array_equal(L2, L0)
    # the held-out predictions of the device's own fit are close to those from the oracle's fit
    _, ao, Lo = O.forward(X, y, params, S, M, gauss_hermite=False)
    ref = R.loo(X, y, ao, Lo, params, S, M, 16)
    print('resident %s: device fit, ratio to the f32 bound %.3g' % (dtype, _ratio32(exp[0], exp[1], ref['mu'], ref['std'], R.row_lmax(ref, N, 16))))
    eng.close()


def _scaled_problem(xalgo, seed=5, N=600):
    """tests/test_gpu_condition.py's problem: an engine trained on scaled data of 4 raw columns, one of them constant"""
    from scfgp_amd.engine import HipEngine
    rng = np.random.default_rng(seed)
    Xr = np.column_stack([rng.uniform(0.5, 3.0, N), rng.gamma(2.0, 1.0, N), np.full(N, 2.5), rng.normal(1.0, 2.0, N)])
    yr = np.exp(0.3 * np.sin(Xr[:, :1]) + 0.1 * Xr[:, 1:2]) + 0.05 * rng.standard_normal((N, 1))
    xs = Scaler(xalgo); xs.fit(Xr); ys = Scaler('normal'); ys.fit(yr)
    D, S, M = 3, 2, 40
    eng = HipEngine(D, S, M, dtype='f64')
    eng.set_params(synth.make_params(seed, D, S, M, abc=(-1.0, 0.0, -4.0)))
    fx = np.ascontiguousarray(xs.forward_transform(Xr)); fy = np.ascontiguousarray(ys.forward_transform(yr))
    eng.set_data(fx, fy)
    _, _, alpha, Li = eng.eval(want_grad=False)
    eng.set_x_scaler(xs)
    return eng, alpha.copy(), Li.copy(), Xr, fx, fy


@pytest.mark.parametrize('xalgo', Scaler.algos)
def test_raw_mode_equals_scaled_mode(xalgo):
    eng, alpha, Li, Xr, fx, fy = _scaled_problem(xalgo)
    rel = lambda a, b: float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b)))
    assert Xr.shape[1] == 4 and fx.shape[1] == 3                                    # the constant column is dropped
    raw = eng.loo(Xr, fy, alpha, Li, block=5, mode='raw')
    sc = eng.loo(fx, fy, alpha, Li, block=5)
    for u, v in zip(raw[:3], sc[:3]):
        assert rel(u, v) < 1e-12
    mu_in, _ = eng.predict(fx, alpha, Li)
    assert rel(sc[0], mu_in) > 1e-6                                                 # holding rows out did move the predictions
    eng.close()


def test_f16x3_equals_fp32_bit_for_bit():
    shape, abc = BIG
    D, S, M, N, block = shape
    params, X, y, alpha, Li = _fit(shape, abc)
    out = []
    for dtype in ('f32', 'f16x3'):
        eng = _engine(D, S, M, dtype, params)
        out.append(eng.loo(X, y, alpha, Li, block=block))
        eng.close()
    for u, v in zip(out[0][:3], out[1][:3]):
        assert np.array_equal(u, v)
    assert out[0][3] == out[1][3]


def test_rows_that_are_not_in_the_fit():
    """factors of a fit on 30 OTHER rows under a weak prior (lam = 2.5e-3, K = 128): the rows of the call lie outside their span, so
    h = phi^T A^-1 phi >> 1 and I - H has no Cholesky factor.  The kernel raises a flag; nothing faults; the context goes on."""
    from scfgp_amd._lib import dptr
    D, S, M, N, block = 5, 4, 60, 400, 7
    params, X, y = R.problem(D, S, M, N, (-3.0, 0.0, -1.0))
    _, a_far, L_far = O.forward(X[300:330], y[300:330], params, S, M, gauss_hermite=False)
    C = O.feature_map(X[:200], params, D, S, M) @ np.tril(L_far).T
    bad = [j for j, (i0, i1) in enumerate(R.blocks(200, block)) if np.linalg.eigvalsh(np.eye(i1 - i0) - C[i0:i1] @ C[i0:i1].T)[0] <= 0]
    assert bad and np.sum(C * C, axis=1).max() >= 1.0
    first = bad[0]
    eng = _engine(D, S, M, 'f64', params)
    with pytest.raises(np.linalg.LinAlgError, match=r'block %d \(rows %d\.\.%d\) is not positive definite' % (first, first * block, first * block + 6)):
        eng.loo(X[:200], y[:200] + 3.0, a_far, L_far, block=block)
    yv = np.ascontiguousarray(y[:200]).ravel(); Xv = np.ascontiguousarray(X[:200]); av = np.ascontiguousarray(a_far).ravel()
    mu = np.empty(200); sd = np.empty(200); stats = np.full(8, 3.0)
    assert eng.lib.scfgp_loo(eng.ctx, dptr(Xv), dptr(yv), 200, dptr(av), dptr(L_far), 0, block, dptr(mu), dptr(sd), None, dptr(stats)) == -3
    assert np.all(stats == 3.0)                                          # untouched
    # the context is still usable: the real fit of these rows
    _, alpha, Li = O.forward(X, y, params, S, M, gauss_hermite=False)
    ref = R.loo(X[:200], y[:200], alpha, Li, params, S, M, block)
    mu, sd, lev, st = eng.loo(X[:200], y[:200], alpha, Li, block=block)
    parity.check_predict(mu, sd, ref['mu'], ref['std'], 'f64')
    eng.close()


def test_errors():
    from scfgp_amd.engine import HipEngine
    from scfgp_amd._lib import dptr
    shape, abc = R.CASES[1]
    D, S, M, N, block = shape
    params, X, y, alpha, Li = _fit(shape, abc)
    eng = _engine(D, S, M, 'f64', params)
    Xv = np.ascontiguousarray(X); yv = np.ascontiguousarray(y).ravel(); av = np.ascontiguousarray(alpha).ravel()
    mu = np.full(N, 3.0); sd = np.full(N, 3.0); stats = np.full(8, 3.0)

    def lib_call(X_, y_, n_, a_, L_, mode, blk, mu_=mu, sd_=sd):
        eng._check(eng.lib.scfgp_loo(eng.ctx, dptr(X_), dptr(y_), n_, dptr(a_), dptr(L_), mode, blk, dptr(mu_), dptr(sd_), None, dptr(stats)), 'loo')
    for args, msg in (((Xv, None, N, av, Li, 0, 7), 'bad arguments'), ((None, yv, N, av, Li, 0, 7), 'bad arguments'),
                      ((Xv, yv, N, None, Li, 0, 7), 'bad arguments'), ((Xv, yv, N, av, None, 0, 7), 'bad arguments'),
                      ((Xv, yv, N, av, Li, 2, 7), 'bad arguments'), ((Xv, yv, N, av, Li, 0, 0), r'block must lie in 1\.\.64'),
                      ((Xv, yv, N, av, Li, 0, 65), r'block must lie in 1\.\.64'), ((Xv, yv, 0, av, Li, 0, 7), 'n must be at least 1'),
                      ((Xv, yv, N, av, Li, 1, 7), 'no X scaler'), ((None, None, 0, av, Li, 0, 7), 'no resident rows'),
                      ((None, None, 0, av, Li, 1, 7), 'mode must be 0')):
        with pytest.raises(ValueError, match=msg):
            lib_call(*args)
    with pytest.raises(ValueError, match='bad arguments'):
        lib_call(Xv, yv, N, av, Li, 0, 7, mu_=None)
    assert np.all(mu == 3.0) and np.all(sd == 3.0) and np.all(stats == 3.0)
    for bad in (np.nan, np.inf):
        yb = yv.copy(); yb[17] = bad
        with pytest.raises(FloatingPointError, match='non-finite'):
            eng.loo(Xv, yb, alpha, Li, block=7)
    Xb = Xv.copy(); Xb[3, 2] = np.nan
    with pytest.raises(FloatingPointError, match='non-finite'):
        lib_call(Xb, yv, N, av, Li, 0, 7)
    Lb = Li.copy(); Lb[50, 3] = np.inf
    with pytest.raises(FloatingPointError, match='non-finite'):
        lib_call(Xv, yv, N, av, Lb, 0, 7)
    assert np.all(stats == 3.0)
    with pytest.raises(ValueError, match='columns'):
        eng.loo(Xv[:, :4], yv, alpha, Li)
    with pytest.raises(ValueError, match='entries'):
        eng.loo(Xv, yv[:-1], alpha, Li)
    with pytest.raises(ValueError, match='shape'):
        eng.loo(Xv, yv, alpha, Li[:-1])
    with pytest.raises(ValueError, match='scaler'):
        eng.loo(Xv, yv, alpha, Li, mode='raw')
    with pytest.raises(ValueError, match='go together'):
        eng.loo(Xv, None, alpha, Li)
    with pytest.raises(ValueError, match='no resident rows'):
        eng.loo(None, None, alpha, Li)
    ref, mu0, sd0 = _ref(shape, abc)
    out = eng.loo(Xv, yv, alpha, Li, block=block)                        # the context still works
    parity.check_predict(out[0], out[1], mu0, sd0, 'f64')
    eng.close()
    fresh = HipEngine(D, S, M, dtype='f64')                              # no parameters yet
    with pytest.raises(ValueError, match='parameters not set'):
        fresh.loo(Xv, yv, alpha, Li)
    fresh.close()


def test_facade(tmp_path):
    from scfgp_amd import SCFGP
    rng = np.random.default_rng(5)
    np.random.seed(5)
    N = 90
    X = rng.uniform(-2, 2, (N, 3))
    X = np.column_stack([X[:, :2], np.full(N, 4.0), X[:, 2:]])          # a constant column
    y = np.sin(X[:, :1]) + 0.5 * X[:, 1:2] ** 2 + 0.05 * rng.standard_normal((N, 1))
    model = SCFGP(sparsity=3, nfeats=12)
    model.fit(X, y, max_iter=15,
              algo={'algo': 'adam', 'algo_params': {'learning_rate': 0.02, 'beta1': 0.9, 'beta2': 0.999, 'epsilon': 1e-8}})
    evals = {k: list(v[1]) for k, v in model.evals.items()}
    a_before, L_before = np.array(model.alpha), np.array(model.Li)
    mu_y, std_y, met = model.loo()
    assert mu_y.shape == (N, 1) and std_y.shape == (N, 1)
    assert {k: list(v[1]) for k, v in model.evals.items()} == evals
    assert np.array_equal(model.alpha, a_before) and np.array_equal(model.Li, L_before)
    # the slow way: one refit per row with the scalers held fixed, then the facade's own back-transform and metrics
    fx, fy = np.asarray(model.X), np.asarray(model.y)
    mu_f = np.empty((N, 1)); sd_f = np.empty(N)
    for i in range(N):
        keep = np.r_[0:i, i + 1:N]
        _, a, L = model.train_func(np.ascontiguousarray(fx[keep]), np.ascontiguousarray(fy[keep]))
        m, s = model.pred_func(np.ascontiguousarray(fx[i:i + 1]), a, L)
        mu_f[i], sd_f[i] = m[0], s[0]
    model.train_func(model.X, model.y)                                   # the training rows are resident again
    bw = model.y_scaler.backward_transform
    mu0 = bw(mu_f); sd0 = 0.5 * (bw(mu_f + sd_f[:, None]) - bw(mu_f - sd_f[:, None]))
    print('facade ratio', parity.predict_ratio(mu_y, std_y, mu0, sd0, 'f64'))
    parity.check_predict(mu_y, std_y, mu0, sd0, 'f64')
    err = mu0 - y
    mae, mse = np.mean(np.abs(err)), np.mean(err ** 2.)
    mnlp = 0.5 * np.mean((err / sd0) ** 2 + np.log(2 * np.pi * sd0 ** 2))
    nmse = mse / np.var(y)
    want = {'MAE': mae, 'NMAE': mae / np.std(y), 'MSE': mse, 'NMSE': nmse, 'MNLP': mnlp, 'SCORE': nmse / (1 + np.exp(-mnlp))}
    assert set(met) == set(want) | {'LOO_LPD'}
    # rows within 1e-9 sigma0 of the refits (the bound above) move these means of smooth functions of them by a few 1e-9 relative
    for k, v in want.items():
        assert abs(met[k] - v) <= 1e-7 * abs(v), (k, met[k], v)
    lpd = np.mean(-0.5 * (((fy - mu_f).ravel() / sd_f) ** 2 + np.log(2 * np.pi * sd_f ** 2)))
    assert abs(met['LOO_LPD'] - lpd) <= 1e-7 * abs(lpd)
    # blocks, and a restored model that holds no rows
    mu_b, std_b, met_b = model.loo(block=9)
    assert not np.allclose(mu_b, mu_y, rtol=1e-9, atol=0)
    path = str(tmp_path / 'model.npz')
    model.save(path)
    fresh = SCFGP(sparsity=3, nfeats=12)
    fresh.load(path)
    assert fresh.X is None
    with pytest.raises(ValueError, match='no training rows'):
        fresh.loo()
    mu_r, std_r, met_r = fresh.loo(X, y, block=9)
    assert np.allclose(mu_r, mu_b, rtol=1e-9, atol=1e-12) and np.allclose(std_r, std_b, rtol=1e-9, atol=1e-12)
    assert abs(met_r['LOO_LPD'] - met_b['LOO_LPD']) <= 1e-9 * abs(met_b['LOO_LPD'])
