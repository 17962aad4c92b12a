"""GPU tier of the posterior update (scfgp_condition): parity of the device update, fed the oracle's fit of the first N0 rows, with the
oracle's fit on all rows under the project's per-tile bounds (tests/parity.py: TOL, unchanged); device fit -> update against the device
fit on all rows; the bit-level guarantees (zeros above the diagonal, aliasing, f16x3 = fp32); the input modes; survival of the training
state; the SCFGP.condition facade on a restored checkpoint; and the errors."""
import functools

import numpy as np
import pytest

from oracle import scfgp_oracle as O
from scfgp_amd import synth
from scfgp_amd.scaler import Scaler
from tests import condition_ref as R
from tests import parity

pytestmark = pytest.mark.gpu

# tests/test_condition_ref.py's shapes and two whose new rows fill one / two chunks of 32 768 and leave a ragged last one (with three
# chunks a half of the upload buffer is reused)
SHAPES = [(5, 4, 60, 1000, 300), (5, 4, 60, 1000, 1), (20, 20, 280, 3000, 700), (64, 32, 1024, 4000, 900), (3, 1, 20, 150, 400),
          (40, 4, 100, 2000, 129), (5, 4, 60, 1000, 32768 + 300), (5, 4, 60, 1000, 65536 + 300)]


@functools.lru_cache(maxsize=None)
def _fits(D, S, M, N0, n):
    params, X, y, Xs = R.problem(D, S, M, N0, n)
    _, a0, L0 = O.forward(X[:N0], y[:N0], params, S, M, gauss_hermite=False)
    _, a1, L1 = O.forward(X, y, params, S, M, gauss_hermite=False)
    mu1, sd1 = O.predict(Xs, a1, L1, params, S, M)
    return params, X, y, Xs, a0, L0, a1, L1, mu1, sd1


def _engine(D, S, M, dtype, params):
    from scfgp_amd.engine import HipEngine
    eng = HipEngine(D, S, M, dtype=dtype); eng.set_params(params)
    return eng


def _checks(eng, al, Li, a1, L1, Xs, mu1, sd1, tol, label):
    mu, sd = eng.predict(Xs, al, Li)
    r = dict(alpha=parity.alpha_ratio(al, a1, tol), Li=parity.li_ratio(Li, L1, tol), predict=parity.predict_ratio(mu, sd, mu1, sd1, tol))
    print(label, tol, parity.fmt(r))
    parity.check_alpha(al, a1, tol); parity.check_li(Li, L1, tol); parity.check_predict(mu, sd, mu1, sd1, tol)
    return r


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('D,S,M,N0,n', SHAPES)
def test_parity_with_the_oracle_fit_on_all_rows(D, S, M, N0, n, dtype):
    """the device update is fed the ORACLE's factors of the first N0 rows, so only the update's own error is measured"""
    params, X, y, Xs, a0, L0, a1, L1, mu1, sd1 = _fits(D, S, M, N0, n)
    eng = _engine(D, S, M, dtype, params)
    al, Li = eng.condition(X[N0:], y[N0:], a0, L0)
    assert al.shape == (2 * (S + M), 1) and Li.shape == L1.shape
    assert np.all(np.triu(Li, 1) == 0.0)                                 # exactly zero above the diagonal
    _checks(eng, al, Li, a1, L1, Xs, mu1, sd1, dtype, 'condition %s' % ((D, S, M, N0, n),))
    assert parity.alpha_ratio(a0, a1, 'f32') > 1.0                       # the unconditioned factors fail even the looser bound
    if n == 1 and dtype == 'f64':
        # one row moves Li by about the fp32 Li bound only: the move itself must be the oracle's (in fp32 mode alpha and predict judge)
        assert np.linalg.norm((Li - L0) - (L1 - L0)) <= 1e-6 * np.linalg.norm(L1 - L0)
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('D,S,M,N0,n', [SHAPES[0], SHAPES[2], SHAPES[6]])
def test_device_fit_then_update_equals_device_fit_on_all_rows(D, S, M, N0, n, dtype):
    params, X, y, Xs, *_ = _fits(D, S, M, N0, n)
    eng = _engine(D, S, M, dtype, params)
    _, _, a0, L0 = eng.eval(np.ascontiguousarray(X[:N0]), np.ascontiguousarray(y[:N0]), want_grad=False)
    al, Li = eng.condition(X[N0:], y[N0:], a0.copy(), L0.copy())
    _, _, a1, L1 = eng.eval(X, y, want_grad=False)
    mu1, sd1 = eng.predict(Xs, a1, L1)
    _checks(eng, al, Li, a1, L1, Xs, mu1, sd1, dtype, 'end to end %s' % ((D, S, M, N0, n),))
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_outputs_may_alias_the_inputs(dtype):
    from scfgp_amd._lib import dptr
    D, S, M, N0, n = SHAPES[2]
    params, X, y, Xs, a0, L0, *_ = _fits(D, S, M, N0, n)
    eng = _engine(D, S, M, dtype, params)
    al, Li = eng.condition(X[N0:], y[N0:], a0, L0)
    # entries above the diagonal of the incoming factor are not read
    al2, Li2 = eng.condition(X[N0:], y[N0:], a0, L0 + np.triu(np.full_like(L0, 7.0), 1))
    assert np.array_equal(al2, al) and np.array_equal(Li2, Li)
    Xn = np.ascontiguousarray(X[N0:]); yn = np.ascontiguousarray(y[N0:]).ravel()
    a = np.ascontiguousarray(a0).ravel().copy(); L = np.ascontiguousarray(L0).copy()
    eng._check(eng.lib.scfgp_condition(eng.ctx, dptr(Xn), dptr(yn), n, dptr(a), dptr(L), 0, dptr(a), dptr(L)), 'condition')
    assert np.array_equal(a, al.ravel()) and np.array_equal(L, Li)
    eng.close()


def test_f16x3_equals_fp32_bit_for_bit():
    D, S, M, N0, n = SHAPES[3]
    params, X, y, Xs, a0, L0, *_ = _fits(D, S, M, N0, n)
    out = []
    for dtype in ('f32', 'f16x3'):
        eng = _engine(D, S, M, dtype, params)
        out.append(eng.condition(X[N0:], y[N0:], a0, L0))
        eng.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def _scaled_problem(xalgo, yalgo, seed=5, N=600, T=50):
    """tests/test_gpu_predict_cov.py's problem: an engine trained on scaled data of 4 raw columns, one of them constant"""
    from scfgp_amd.engine import HipEngine
    rng = np.random.default_rng(seed)
    Xr = np.column_stack([rng.uniform(0.5, 3.0, N + T), rng.gamma(2.0, 1.0, N + T), np.full(N + T, 2.5), rng.normal(1.0, 2.0, N + T)])
    yr = np.exp(0.3 * np.sin(Xr[:, :1]) + 0.1 * Xr[:, 1:2]) + 0.05 * rng.standard_normal((N + T, 1))
    xs = Scaler(xalgo); xs.fit(Xr[:N]); ys = Scaler(yalgo); ys.fit(yr[:N])
    D, S, M = 3, 2, 40
    eng = HipEngine(D, S, M, dtype='f64')
    eng.set_params(synth.make_params(seed, D, S, M, abc=(-1.0, 0.0, -4.0)))
    eng.set_data(np.ascontiguousarray(xs.forward_transform(Xr[:N])), np.ascontiguousarray(ys.forward_transform(yr[:N])))
    _, _, alpha, Li = eng.eval(want_grad=False)
    eng.set_x_scaler(xs); eng.set_y_scaler(ys)
    return eng, xs, ys, alpha.copy(), Li.copy(), Xr[N:], yr[N:]


@pytest.mark.parametrize('xalgo', Scaler.algos)
def test_raw_mode_equals_scaled_mode(xalgo):
    """the device's transform of a raw column against the host's: the 1e-12 of tests/test_gpu_predict_cov.py's test of the same name
    (both are fp64 evaluations of the same element-wise formula; the update that follows is the same code on inputs that close)"""
    eng, xs, ys, alpha, Li, Xr, yr = _scaled_problem(xalgo, 'normal')
    rel = lambda a, b: float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))
    yn = ys.forward_transform(yr)
    fx = np.ascontiguousarray(xs.forward_transform(Xr))
    assert Xr.shape[1] == 4 and fx.shape[1] == 3                                    # the constant column is dropped
    ar, Lr = eng.condition(Xr, yn, alpha, Li, mode='raw')
    a0, L0 = eng.condition(fx, yn, alpha, Li)
    assert rel(ar, a0) < 1e-12 and rel(Lr, L0) < 1e-12
    assert rel(a0, alpha) > 1e-6                                                    # the rows did move the posterior
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_training_state_survives(dtype):
    from scfgp_amd.engine import HipEngine
    D, S, M = 20, 20, 280
    params = synth.make_params(7, D, S, M, abc=(-1.0, 0.0, -1.0))
    X = synth.make_X(7, 1500, D)
    y = np.sin(3 * X[:, :1]) + 0.1 * synth.normal(10, 0, 1500)[:, None]
    Xn = synth.make_X(9, 33000, D); yn = np.sin(3 * Xn[:, 0])
    eng = HipEngine(D, S, M, dtype=dtype); eng.set_params(params); eng.set_data(X, y)
    c0, g0, a0, L0 = eng.eval(want_grad=True)
    c0, g0, a0, L0 = float(c0), g0.copy(), a0.copy(), L0.copy()
    eng.condition(Xn, yn, a0, L0)
    eng.condition(Xn[:7], yn[:7], a0, L0)
    c1, g1, a1, L1 = eng.eval(want_grad=True)
    assert float(c1) == c0 and np.array_equal(g1, g0) and np.array_equal(a1, a0) and np.array_equal(L1, L0)
    eng.close()
    # two successive scfgp_train calls, with and without an update between them
    runs = []
    for between in (False, True):
        eng = HipEngine(D, S, M, dtype=dtype); eng.set_params(params); eng.set_data(X, y)
        eng.opt_init('adam', learning_rate=0.01)
        h1, al, Li = eng.train(3)
        if between:
            eng.condition(Xn[:5000], yn[:5000], al, Li)
        h2, al2, Li2 = eng.train(3)
        runs.append((h1.copy(), h2.copy(), eng.get_params().copy(), al2.copy(), Li2.copy()))
        eng.close()
    for u, v in zip(*runs):
        assert np.array_equal(u, v)


def test_facade_condition_on_a_restored_checkpoint(tmp_path):
    from scfgp_amd import SCFGP
    rng = np.random.default_rng(5)
    np.random.seed(5)
    X = rng.uniform(-2, 2, (400, 3))
    X = np.column_stack([X[:, :2], np.full(400, 4.0), X[:, 2:]])     # a constant column
    y = np.sin(X[:, :1]) + 0.5 * X[:, 1:2] ** 2 + 0.05 * rng.standard_normal((400, 1))
    N0 = 240
    model = SCFGP(sparsity=3, nfeats=12, device_scaler=True)
    model.fit(X[:N0], y[:N0], max_iter=20,
              algo={'algo': 'adam', 'algo_params': {'learning_rate': 0.02, 'beta1': 0.9, 'beta2': 0.999, 'epsilon': 1e-8}})
    path = str(tmp_path / 'model.npz')
    model.save(path)
    fresh = SCFGP(sparsity=3, nfeats=12, device_scaler=True)
    fresh.load(path)                                                   # never saw set_data: no rows
    assert fresh.X is None
    a_old = np.array(fresh.alpha)
    assert fresh.condition(X[N0:340], y[N0:340]) is fresh
    assert fresh.X is None and not np.array_equal(fresh.alpha, a_old)
    # the reference: train_func on all 340 rows scaled with the SAME fitted scalers
    fx = np.ascontiguousarray(model.X_scaler.forward_transform(X[:340]), dtype=np.float64)
    fy = np.ascontiguousarray(model.y_scaler.forward_transform(y[:340]), dtype=np.float64)
    _, a1, L1 = model.train_func(fx, fy)
    Xs = np.ascontiguousarray(model.X_scaler.forward_transform(X[340:]), dtype=np.float64)
    mu1, sd1 = model.pred_func(Xs, a1, L1)
    mu, sd = fresh.pred_func(Xs, fresh.alpha, fresh.Li)
    print('facade predict ratio', parity.predict_ratio(mu, sd, mu1, sd1, 'f64'))
    parity.check_predict(mu, sd, mu1, sd1, 'f64')
    smp = fresh.sample(X[340:], 8, seed=3)
    assert smp.shape == (60, 8) and np.all(np.isfinite(smp))
    cov = fresh.predict_cov(X[340:])
    assert cov.shape == (60, 60) and np.all(np.isfinite(cov))
    other = SCFGP(sparsity=3, nfeats=12)
    other.pred_func = lambda Xs, alpha, Li: None
    with pytest.raises(TypeError):
        other.condition(X[:5], y[:5])


def test_errors():
    from scfgp_amd.engine import HipEngine
    from scfgp_amd._lib import dptr
    D, S, M, N0, n = SHAPES[0]
    params, X, y, Xs, a0, L0, a1, L1, mu1, sd1 = _fits(D, S, M, N0, n)
    eng = _engine(D, S, M, 'f64', params)
    Xn = np.ascontiguousarray(X[N0:]); yn = np.ascontiguousarray(y[N0:]).ravel()
    a = np.ascontiguousarray(a0).ravel()
    ao = np.full(a.size, 3.0); Lo = np.full(L0.shape, 3.0)

    def lib_call(Xn_, yn_, n_, a_, L_, mode):
        eng._check(eng.lib.scfgp_condition(eng.ctx, dptr(Xn_), dptr(yn_), n_, dptr(a_), dptr(L_), mode, dptr(ao), dptr(Lo)), 'condition')
    for bad in (np.nan, np.inf):
        yb = yn.copy(); yb[17] = bad
        with pytest.raises(FloatingPointError, match='non-finite'):
            lib_call(Xn, yb, n, a, L0, 0)
        with pytest.raises(FloatingPointError, match='non-finite'):
            eng.condition(Xn, yb, a0, L0)
    Xb = Xn.copy(); Xb[3, 2] = np.nan
    with pytest.raises(FloatingPointError, match='non-finite'):
        lib_call(Xb, yn, n, a, L0, 0)
    Lb = L0.copy(); Lb[50, 3] = np.inf
    with pytest.raises(FloatingPointError, match='non-finite'):
        lib_call(Xn, yn, n, a, Lb, 0)
    with pytest.raises(ValueError, match='n must be at least 1'):
        lib_call(Xn, yn, 0, a, L0, 0)
    with pytest.raises(ValueError, match='bad arguments'):
        lib_call(Xn, yn, n, a, L0, 2)
    with pytest.raises(ValueError, match='bad arguments'):
        lib_call(Xn, None, n, a, L0, 0)
    with pytest.raises(ValueError, match='no X scaler'):
        lib_call(Xn, yn, n, a, L0, 1)
    assert np.all(ao == 3.0) and np.all(Lo == 3.0)                       # the outputs are untouched by every failure
    with pytest.raises(ValueError, match='columns'):
        eng.condition(Xn[:, :4], yn, a0, L0)
    with pytest.raises(ValueError, match='entries'):
        eng.condition(Xn, yn[:-1], a0, L0)
    with pytest.raises(ValueError, match='shape'):
        eng.condition(Xn, yn, a0, L0[:-1])
    with pytest.raises(ValueError, match='scaler'):
        eng.condition(Xn, yn, a0, L0, mode='raw')
    with pytest.raises(ValueError):
        eng.condition(Xn, yn, a0, L0, mode='y')
    assert isinstance(eng.condition(), dict)                             # without arguments: the condition estimate, as before
    al, Li = eng.condition(Xn, yn, a0, L0)                               # the context still works
    _checks(eng, al, Li, a1, L1, Xs, mu1, sd1, 'f64', 'after the errors')
    eng.close()
    fresh = HipEngine(D, S, M, dtype='f64')                              # no parameters yet
    with pytest.raises(ValueError, match='parameters not set'):
        fresh.condition(Xn, yn, a0, L0)
    fresh.close()
