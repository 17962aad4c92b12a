"""GPU tier of the posterior covariance of the input gradient (gradcov.hip: scfgp_predict_gradcov): parity with the numpy closed form
(tests/gradcov_ref.py) over the geometry classes of q = min(D, S), multi-chunk calls with the chunk boundaries placed by
HipEngine.gradcov_points_per_chunk, the bit-level promises of include/scfgp_hip.h, raw mode through every X scaler, every combination
of outputs, the refusals, and the SCFGP facade (predict_gradcov, active_subspace).  Every geometry here has K <= 172: the 128-wide
column plan of K > 256, K = 256 = Kp, the factors of a real fit and a context that other entry points share are covered by the geometry
sweep and the stale-state sequences (tests/test_gpu_posterior_geometry.py, tests/test_gpu_posterior_sequence.py)."""
import itertools

import numpy as np
import pytest

from scfgp_amd import synth
from scfgp_amd._lib import dptr
from scfgp_amd.scaler import Scaler
from tests import gradcov_ref as R
from tests import pred_grad_ref as PG

pytestmark = pytest.mark.gpu

# dvar, dcov, asub: BOUNDS of tests/test_gpu_predict_cov.py -- the factor comes from the same apply_c and is squared in the same bilinear
# form.  dmu: the first entry of tests/test_gpu_predict_grad.py's BOUNDS.
BOUNDS = {'f64': 1e-10, 'f32': 6e-6}
BOUNDS_DMU = {'f64': 1e-10, 'f32': 3e-5}
ALL = ('dmu', 'dvar', 'dcov', 'asub')


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def _engine(D, S, M, dtype):
    from scfgp_amd.engine import HipEngine
    params, alpha, Li = R.synthetic(D, S, M)
    eng = HipEngine(D, S, M, dtype=dtype); eng.set_params(params)
    return eng, params, alpha, Li


def _reference(Xs, alpha, Li, params, S, M, w=None, block=256):
    """m, diag Sigma and the sums of asub of all rows, block by block (the T x K x D Jacobian of a long call does not fit)"""
    T, D = Xs.shape
    m = np.empty((T, D)); dv = np.empty((T, D)); acc = np.zeros((D, D))
    w = np.ones(T) if w is None else w
    for t0 in range(0, T, block):
        sl = slice(t0, min(T, t0 + block))
        mm, Sig = R.gradcov(Xs[sl], alpha, Li, params, S, M)
        m[sl] = mm; dv[sl] = np.diagonal(Sig, axis1=1, axis2=2)
        acc += np.einsum('t,tde->de', w[sl], mm[:, :, None] * mm[:, None, :] + Sig)
    return m, dv, acc / w.sum()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('D,S,M', R.GEOMETRIES)
def test_parity_over_the_geometry_classes(D, S, M, dtype):
    eng, params, alpha, Li = _engine(D, S, M, dtype)
    Xs = R.points(D)
    T = len(Xs)
    w = 0.25 + synth.uniform(77, 0, T)
    out = eng.predict_gradcov(Xs, alpha, Li, w=w, want=ALL)
    assert out['dmu'].shape == (T, D) and out['dvar'].shape == (T, D) and out['dcov'].shape == (T, D, D) and out['asub'].shape == (D, D)
    m, Sig = R.gradcov(Xs, alpha, Li, params, S, M)
    errs = dict(dmu=rel(out['dmu'], m), dvar=rel(out['dvar'], np.diagonal(Sig, axis1=1, axis2=2)), dcov=rel(out['dcov'], Sig),
                asub=rel(out['asub'], R.asub(m, Sig, w)))
    print('parity T=%d' % T, (D, S, M), dtype, ' '.join('%s=%.2e' % kv for kv in errs.items()))
    assert errs['dmu'] < BOUNDS_DMU[dtype], errs
    assert max(errs['dvar'], errs['dcov'], errs['asub']) < BOUNDS[dtype], errs
    assert np.all(out['dvar'] >= 0)
    # T = 1: the same point alone, bit for bit (promise 2), and its own parity
    one = eng.predict_gradcov(Xs[100:101], alpha, Li, want=ALL)
    for k in ('dmu', 'dvar', 'dcov'):
        assert np.array_equal(one[k][0], out[k][100]), k
    e1 = rel(one['asub'], np.outer(m[100], m[100]) + Sig[100])
    print('parity T=1', (D, S, M), dtype, 'asub=%.2e' % e1)
    assert e1 < BOUNDS[dtype]
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_three_chunks_parity_repeatability_and_trailing_zero_weights(dtype):
    """(70, 5, 60): 12 points per group; asub's records put the chunk at the slot budget.  Promises 2 and 5."""
    D, S, M = 70, 5, 60
    eng, params, alpha, Li = _engine(D, S, M, dtype)
    n = eng.gradcov_points_per_chunk(True)
    assert n == (64 << 20) // (8 * D * D) and eng.gradcov_points_per_chunk(False) == 32768 // 60 * 12
    T = 2 * n + 3
    Xs = synth.make_X(303, T, D)
    w = 0.25 + synth.uniform(78, 0, T)
    out = eng.predict_gradcov(Xs, alpha, Li, w=w)
    assert sorted(out) == ['asub', 'dmu', 'dvar']
    m, dv, A = _reference(Xs, alpha, Li, params, S, M, w)
    errs = (rel(out['dmu'], m), rel(out['dvar'], dv), rel(out['asub'], A))
    print('three chunks', dtype, 'np=%d T=%d dmu=%.2e dvar=%.2e asub=%.2e' % ((n, T) + errs))
    assert errs[0] < BOUNDS_DMU[dtype] and max(errs[1:]) < BOUNDS[dtype], errs
    again = eng.predict_gradcov(Xs, alpha, Li, w=w)
    for k in out:
        assert np.array_equal(out[k], again[k]), k
    for t in (n - 1, n, 2 * n):                                   # around the chunk boundaries: the point alone
        one = eng.predict_gradcov(Xs[t:t + 1], alpha, Li, want=('dmu', 'dvar'))
        assert np.array_equal(one['dmu'][0], out['dmu'][t]) and np.array_equal(one['dvar'][0], out['dvar'][t]), t
    # without a D x D array per point the chunks are longer: the same bits per point
    long_chunks = eng.predict_gradcov(Xs, alpha, Li, want=('dmu', 'dvar'))
    assert np.array_equal(long_chunks['dvar'], out['dvar']) and np.array_equal(long_chunks['dmu'], out['dmu'])
    # rows of weight 0 behind the last weighted row do not change asub
    k0 = n - 2
    wz = w.copy(); wz[k0:] = 0.0
    a_all = eng.predict_gradcov(Xs, alpha, Li, w=wz, want=('asub',))['asub']
    a_head = eng.predict_gradcov(Xs[:k0], alpha, Li, w=w[:k0], want=('asub',))['asub']
    assert np.array_equal(a_all, a_head)
    assert np.array_equal(a_all, a_all.T)
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('D,S,M', [(40, 33, 20), (70, 5, 60)])
def test_three_chunks_with_the_full_covariance(D, S, M, dtype):
    """dcov across three chunks: at (40, 33, 20) one point per group and the chunk is the 32 768-row buffers' 992 points, at (70, 5, 60)
    it is the 64 MiB slot's.  The points around the boundaries equal the same point alone, bit for bit (promise 2)."""
    eng, params, alpha, Li = _engine(D, S, M, dtype)
    n = eng.gradcov_points_per_chunk(True)
    q = min(D, S)
    assert n == min(32768 // (64 // q * q) * (64 // q), (64 << 20) // (8 * D * D))
    T = 2 * n + 3
    Xs = synth.make_X(404, T, D)
    out = eng.predict_gradcov(Xs, alpha, Li, want=('dvar', 'dcov'))
    sel = np.r_[0:8, n - 4:n + 4, 2 * n - 4:2 * n + 3]
    _, Sig = R.gradcov(Xs[sel], alpha, Li, params, S, M)
    e = rel(out['dcov'][sel], Sig)
    print('three chunks dcov', (D, S, M), dtype, 'np=%d T=%d dcov=%.2e' % (n, T, e))
    assert e < BOUNDS[dtype]
    assert np.array_equal(out['dcov'], out['dcov'].transpose(0, 2, 1))
    assert np.array_equal(out['dvar'], np.diagonal(out['dcov'], axis1=1, axis2=2))
    for t in (n - 1, n, 2 * n):
        one = eng.predict_gradcov(Xs[t:t + 1], alpha, Li, want=('dvar', 'dcov'))
        assert np.array_equal(one['dcov'][0], out['dcov'][t]) and np.array_equal(one['dvar'][0], out['dvar'][t]), t
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('D,S,M', [(7, 12, 3), (70, 5, 60), (65, 64, 8)])
def test_bit_level_promises(D, S, M, dtype):
    eng, params, alpha, Li = _engine(D, S, M, dtype)
    Xs = R.points(D)
    w = 0.25 + synth.uniform(79, 0, len(Xs))
    out = eng.predict_gradcov(Xs, alpha, Li, w=w, want=ALL)
    assert np.array_equal(out['dmu'], eng.predict_grad(Xs, alpha, Li, want_std=False)[2])           # 1
    assert np.array_equal(out['dmu'], eng.predict_grad(Xs, alpha, Li)[2])
    assert np.array_equal(out['dcov'], out['dcov'].transpose(0, 2, 1))                              # 3
    assert np.array_equal(out['dvar'], np.diagonal(out['dcov'], axis1=1, axis2=2))
    assert np.array_equal(out['asub'], out['asub'].T)                                               # 4
    # 2: a point's position in its group and in the call does not matter
    part = eng.predict_gradcov(Xs[37:200], alpha, Li, want=('dvar', 'dcov'))
    assert np.array_equal(part['dcov'], out['dcov'][37:200]) and np.array_equal(part['dvar'], out['dvar'][37:200])
    eng.close()


def test_f16x3_context_equals_fp32_context():
    from scfgp_amd.engine import HipEngine
    for D, S, M in ((70, 5, 60), (15, 15, 60)):
        e32, params, alpha, Li = _engine(D, S, M, 'f32')
        e16 = HipEngine(D, S, M, dtype='f16x3'); e16.set_params(params)
        Xs = R.points(D)
        a = e32.predict_gradcov(Xs, alpha, Li, want=ALL)
        b = e16.predict_gradcov(Xs, alpha, Li, want=ALL)
        for k in ALL:
            assert np.array_equal(a[k], b[k]), k
        e32.close(); e16.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_every_combination_of_outputs_gives_the_same_bits(dtype):
    D, S, M = 70, 5, 60
    eng, params, alpha, Li = _engine(D, S, M, dtype)
    Xs = R.points(D)
    w = 0.25 + synth.uniform(80, 0, len(Xs))
    full = eng.predict_gradcov(Xs, alpha, Li, w=w, want=ALL)
    for r in (1, 2, 3):
        for want in itertools.combinations(ALL, r):
            out = eng.predict_gradcov(Xs, alpha, Li, w=w, want=want)
            assert sorted(out) == sorted(want)
            for k in want:
                assert np.array_equal(out[k], full[k]), (want, k)
    eng.close()


def _raw_engine(xalgo):
    from scfgp_amd.engine import HipEngine
    (D, S, M), xs, (params, alpha, Li), Xr = R.raw_problem(xalgo)
    eng = HipEngine(D, S, M, dtype='f64'); eng.set_params(params); eng.set_x_scaler(xs)
    return eng, xs, (D, S, M), params, alpha, Li, Xr


@pytest.mark.parametrize('xalgo', Scaler.algos)
def test_raw_mode_through_every_x_scaler(xalgo):
    eng, xs, (D, S, M), params, alpha, Li, Xr = _raw_engine(xalgo)
    T = len(Xr)
    w = 0.25 + synth.uniform(81, 0, T)
    raw = eng.predict_gradcov(Xr, alpha, Li, w=w, mode='raw', want=ALL)
    cols = list(xs.data['cols'])
    assert cols == [0, 1, 3]
    assert raw['dmu'].shape == (T, 4) and raw['dvar'].shape == (T, 4) and raw['dcov'].shape == (T, 4, 4) and raw['asub'].shape == (4, 4)
    # the dropped constant column: zero rows and columns
    assert np.all(raw['dmu'][:, 2] == 0) and np.all(raw['dvar'][:, 2] == 0)
    assert np.all(raw['dcov'][:, 2, :] == 0) and np.all(raw['dcov'][:, :, 2] == 0)
    assert np.all(raw['asub'][2, :] == 0) and np.all(raw['asub'][:, 2] == 0)
    assert np.array_equal(raw['dmu'], eng.predict_grad(Xr, alpha, Li, mode='raw', want_std=False)[2])       # promise 1 in raw mode
    assert np.array_equal(raw['dcov'], raw['dcov'].transpose(0, 2, 1)) and np.array_equal(raw['asub'], raw['asub'].T)
    assert np.array_equal(raw['dvar'], np.diagonal(raw['dcov'], axis1=1, axis2=2))
    # the scaled call chained by the scaler's derivative on the host
    sc = eng.predict_gradcov(np.ascontiguousarray(xs.forward_transform(Xr)), alpha, Li, want=('dmu', 'dvar', 'dcov'))
    g = PG.x_scaler_deriv(xs, Xr)
    m, Sig = sc['dmu'] * g, sc['dcov'] * g[:, :, None] * g[:, None, :]
    ix = np.ix_(cols, cols)
    assert rel(raw['dmu'][:, cols], m) < 1e-12
    assert rel(raw['dvar'][:, cols], sc['dvar'] * g * g) < 1e-12
    assert rel(raw['dcov'][:, cols][:, :, cols], Sig) < 1e-12
    assert rel(raw['asub'][ix], R.asub(m, Sig, w)) < 1e-12
    # and the closed form itself
    m0, S0 = R.gradcov(xs.forward_transform(Xr), alpha, Li, params, S, M, g=g)
    assert rel(raw['dcov'][:, cols][:, :, cols], S0) < BOUNDS['f64'] and rel(raw['asub'][ix], R.asub(m0, S0, w)) < BOUNDS['f64']
    eng.close()


def test_refusals_leave_the_outputs_untouched_and_the_context_working():
    from scfgp_amd.engine import HipEngine
    D, S, M = 5, 4, 60
    eng, params, alpha, Li = _engine(D, S, M, 'f64')
    T = 10
    Xs = synth.make_X(3, T, D)
    bufs = [np.full((T, D), 7.0), np.full((T, D), 7.0), np.full((T, D, D), 7.0), np.full((D, D), 7.0)]
    o = [dptr(b) for b in bufs]
    fn = eng.lib.scfgp_predict_gradcov

    def refused(match, *args):
        with pytest.raises(ValueError, match=match):
            eng._check(fn(eng.ctx, *args), 'predict_gradcov')
        assert all(np.all(b == 7.0) for b in bufs)

    refused('bad arguments', None, T, None, dptr(alpha), dptr(Li), 0, *o)
    refused('bad arguments', dptr(Xs), T, None, None, dptr(Li), 0, *o)
    refused('bad arguments', dptr(Xs), T, None, dptr(alpha), None, 0, *o)
    refused('bad arguments', dptr(Xs), 0, None, dptr(alpha), dptr(Li), 0, *o)
    refused('bad arguments', dptr(Xs), T, None, dptr(alpha), dptr(Li), 2, *o)
    refused('no output', dptr(Xs), T, None, dptr(alpha), dptr(Li), 0, None, None, None, None)
    refused('no X scaler', dptr(Xs), T, None, dptr(alpha), dptr(Li), 1, *o)
    w = np.ones(T)
    for bad in (-1e-300, np.nan, np.inf):
        wb = w.copy(); wb[T - 1] = bad
        refused('weight 9', dptr(Xs), T, dptr(wb), dptr(alpha), dptr(Li), 0, *o)
    refused('sum to zero', dptr(Xs), T, dptr(np.zeros(T)), dptr(alpha), dptr(Li), 0, *o)
    # w is read only when asub is given
    wb = w.copy(); wb[0] = -1.0
    assert fn(eng.ctx, dptr(Xs), T, dptr(wb), dptr(alpha), dptr(Li), 0, o[0], o[1], o[2], None) == 0
    assert np.all(bufs[3] == 7.0) and not np.any(bufs[2] == 7.0)
    with pytest.raises(ValueError):
        eng.predict_gradcov(Xs, alpha, Li, mode='y')                                                # no raw-y mode
    with pytest.raises(ValueError):
        eng.predict_gradcov(Xs, alpha, Li, want=())
    with pytest.raises(ValueError, match='scaler'):
        eng.predict_gradcov(Xs, alpha, Li, mode='raw')
    mu, sd = eng.predict(Xs, alpha, Li)                                                             # the context still works
    from oracle import scfgp_oracle as O
    mu0, sd0 = O.predict(Xs, alpha[:, None], Li, params, S, M)
    assert rel(mu, mu0) < 1e-10 and rel(sd, sd0) < 1e-10
    eng.close()
    fresh = HipEngine(D, S, M, dtype='f64')                                                        # no parameters yet
    with pytest.raises(ValueError, match='parameters not set'):
        fresh.predict_gradcov(Xs, alpha, Li)
    fresh.close()
    big, bparams, balpha, bLi = _engine(65, 65, 4, 'f64')                                           # min(D, S) = 65
    Xb = synth.make_X(4, 3, 65)
    with pytest.raises(ValueError, match='at most 64'):
        big.predict_gradcov(Xb, balpha, bLi)
    mu, sd = big.predict(Xb, balpha, bLi)
    mu0, sd0 = O.predict(Xb, balpha[:, None], bLi, bparams, 65, 4)
    assert rel(mu, mu0) < 1e-10 and rel(sd, sd0) < 1e-10
    big.close()


def _fit(X, y, S, M, iters, dtype='f64'):
    from scfgp_amd import SCFGP
    np.random.seed(5)
    model = SCFGP(sparsity=S, nfeats=M, device_scaler=True, dtype=dtype)
    n = len(X) * 4 // 5
    model.set_data(X[:n], y[:n])
    model.optimize(X[n:], y[n:], max_iter=iters,
                   algo={'algo': 'adam', 'algo_params': {'learning_rate': 0.02, 'beta1': 0.9, 'beta2': 0.999, 'epsilon': 1e-8}})
    return model, X[n:]


def test_facade_predict_gradcov():
    from scfgp_amd import SCFGP
    rng = np.random.default_rng(5)
    X = rng.uniform(-2, 2, (300, 3))
    X = np.column_stack([X[:, :2], np.full(300, 4.0), X[:, 2:]])     # a constant column
    y = np.sin(X[:, :1]) + 0.5 * X[:, 1:2] ** 2 + 0.05 * rng.standard_normal((300, 1))
    model, Xs = _fit(X, y, 3, 12, 20)
    T = len(Xs)
    mean, std = model.predict_gradcov(Xs)
    mean2, std2, cov = model.predict_gradcov(Xs, full=True)
    assert mean.shape == (T, 4) and std.shape == (T, 4) and cov.shape == (T, 4, 4)
    assert np.array_equal(mean, mean2) and np.array_equal(std, std2)
    assert np.all(mean[:, 2] == 0) and np.all(std[:, 2] == 0) and np.all(cov[:, 2] == 0) and np.all(cov[:, :, 2] == 0)
    eng = model.pred_func.__self__.engine
    out = eng.predict_gradcov(Xs, model.alpha, model.Li, mode='raw', want=('dmu', 'dvar', 'dcov'))
    assert np.array_equal(mean, out['dmu']) and np.array_equal(std, np.sqrt(out['dvar'])) and np.array_equal(cov, out['dcov'])
    # the mean: central differences of the scaled mean in the raw inputs (the step and the bound of tests/test_gpu_predict_grad.py) ...
    cols = [0, 1, 3]
    h = 1e-6
    fd = np.zeros((T, 4))
    for c in cols:
        hh = h * max(1.0, abs(Xs[:, c]).max())
        Xp = Xs.copy(); Xp[:, c] += hh
        Xm = Xs.copy(); Xm[:, c] -= hh
        fd[:, c] = (eng.predict_raw(Xp, model.alpha, model.Li)[0] - eng.predict_raw(Xm, model.alpha, model.Li)[0]).ravel() / (2 * hh)
    assert rel(mean, fd) < 1e-5
    # ... and SCFGP.predict_grad's mean gradient, which is this one through the y scaler's backward transform
    mu_s = eng.predict_raw(Xs, model.alpha, model.Li)[0]
    dmu_y = model.predict_grad(Xs)[2]
    assert rel(PG.y_backward_deriv(model.y_scaler, mu_s) * mean, dmu_y) < 1e-10
    other = SCFGP(sparsity=3, nfeats=12)
    other.pred_func = lambda Xs, alpha, Li: None
    with pytest.raises(TypeError):
        other.predict_gradcov(Xs)
    with pytest.raises(TypeError):
        other.active_subspace(Xs)


def _subspace_angle(U, V):
    """largest principal angle between the column spaces of U and V"""
    Qu, _ = np.linalg.qr(U); Qv, _ = np.linalg.qr(V)
    s = np.linalg.svd(Qu.T @ Qv, compute_uv=False)
    return float(np.arccos(np.clip(s.min(), -1.0, 1.0)))


def test_facade_active_subspace_finds_the_two_directions_of_the_target():
    """y depends on x through a . x and b . x only.  The bound on the device's subspace angle is the CPU closed form's own angle on
    this fit plus the perturbation an fp32-sized relative error of asub can cause (Davis-Kahan: sin theta <= ||E|| / gap, E <= 6e-6
    ||asub||, gap = lambda_2 - lambda_3 of the reference); the fit runs in fp64, so this is generous.  That the fitted surrogate has
    found the directions at all is asserted on the reference: its angle is under 0.35 rad (20 degrees)."""
    rng = np.random.default_rng(8)
    D = 6
    a = np.array([1.0, -1.0, 0.5, 0.0, 0.0, 0.0]); b = np.array([0.0, 0.5, 1.0, 1.0, 0.0, 0.0])
    X = rng.uniform(-1, 1, (1000, D))
    y = (np.sin(1.5 * X @ a) + 0.5 * (X @ b) ** 2)[:, None] + 0.02 * rng.standard_normal((1000, 1))
    model, Xs = _fit(X, y, 4, 40, 150)
    lam, vec, A = model.active_subspace(Xs)
    assert lam.shape == (D,) and vec.shape == (D, D) and A.shape == (D, D)
    assert np.all(np.diff(lam) <= 0) and np.array_equal(A, A.T)
    assert rel(vec @ np.diag(lam) @ vec.T, A) < 1e-12
    # the reference on the same fit
    params = model.params.get_value()
    fx = model.X_scaler.forward_transform(Xs)
    m0, S0 = R.gradcov(fx, model.alpha, model.Li, params, model.S, model.M, g=PG.x_scaler_deriv(model.X_scaler, Xs))
    A0 = R.asub(m0, S0)
    l0, v0 = np.linalg.eigh(A0)
    l0, v0 = l0[::-1], v0[:, ::-1]
    truth = np.column_stack([a, b])
    th0 = _subspace_angle(v0[:, :2], truth)
    th = _subspace_angle(vec[:, :2], truth)
    slack = float(np.arcsin(min(1.0, 6e-6 * l0[0] / (l0[1] - l0[2]))))
    print('active subspace: reference angle %.4f rad, device %.4f, slack %.2e, eigenvalues %s' % (th0, th, slack, l0))
    print('active subspace: asub against the reference %.2e' % rel(A, A0))
    assert th0 < 0.35
    assert th <= th0 + slack
    # weights: the rows of weight zero do not count
    w = np.r_[np.ones(len(Xs) // 2), np.zeros(len(Xs) - len(Xs) // 2)]
    assert np.array_equal(model.active_subspace(Xs, w=w)[2], model.active_subspace(Xs[:len(Xs) // 2])[2])
