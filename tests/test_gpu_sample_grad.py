"""GPU tier of scfgp_sample_grad (samplegrad.hip): values and input gradients of sample functions, one sample per row, against the numpy
closed form (tests/sample_grad_ref.py); bit-for-bit agreement with scfgp_predict_grad's mean gradient and position independence; the
agreement of val with scfgp_sample; the three input modes through every scaler; the argument errors with untouched outputs; survival of
the training state; and the SCFGP.sample_maximize facade."""
import numpy as np
import pytest

from scfgp_amd import synth
from scfgp_amd.scaler import Scaler
from tests import pred_grad_ref as G
from tests import sample_grad_ref as R
from tests import sample_ref as SR

pytestmark = pytest.mark.gpu

CHUNK = 32768
# (D, S, M, T): J = 21 odd (unaligned sine half, ragged last feature step, ragged rows) | two 16-wide D tiles | nine D tiles (launch plan
# 8 + 1) | the chunk boundary
SHAPES = [(3, 1, 20, 700), (20, 4, 60, 301), (130, 2, 30, 97), (5, 4, 60, CHUNK + 500)]
GRAD_BOUNDS = {'f64': 1e-10, 'f32': 3e-5}            # predict_grad's dmu (tests/test_gpu_predict_grad.py)
VAL_BOUNDS = {'f64': 1e-10, 'f32': 3e-6}             # scfgp_sample (tests/test_gpu_sample.py)
NSAMPS = (1, 7, 300, 1024)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def _synthetic(D, S, M, dtype):
    """an engine with parameters set and synthetic alpha / Li, as tests/test_gpu_sample.py builds it"""
    from scfgp_amd.engine import HipEngine
    seed = 0x5CF65000 + M
    K = 2 * (S + M)
    params = synth.make_params(seed + 0x0202, D, S, M, abc=(-1.0, 0.0, -1.0))
    rng = np.random.default_rng(seed)
    alpha = rng.standard_normal(K) / np.sqrt(K)
    Li = np.tril(rng.standard_normal((K, K))) / np.sqrt(K)
    eng = HipEngine(D, S, M, dtype=dtype); eng.set_params(params)
    return eng, params, alpha, Li


def _rows(T):
    """both ends, the middle and both sides of every chunk boundary"""
    parts = [np.arange(0, 40), np.arange(T // 2, T // 2 + 40), np.arange(T - 40, T)]
    for b in range(CHUNK, T, CHUNK):
        parts.append(np.arange(b - 40, b + 40))
    sel = np.unique(np.concatenate(parts))
    return sel[(sel >= 0) & (sel < T)]


def _sidx_kinds(T, nsamp, rng):
    return (('random', rng.integers(0, nsamp, T)), ('last', np.full(T, nsamp - 1, dtype=np.int64)), ('null', None))


def _check_against_reference(eng, params, alpha, Li, S, M, Xs, dtype, nsamps=NSAMPS):
    T = Xs.shape[0]
    sel = _rows(T)
    rng = np.random.default_rng(T)
    for ns in nsamps:
        W = SR.weights(alpha, Li, SR.kappa(params), ns, 9)
        for kind, sidx in _sidx_kinds(T, ns, rng):
            val, grad = eng.sample_grad(Xs, W, sidx=sidx)
            assert val.shape == (T,) and grad.shape == Xs.shape
            s_ref = (sel % ns) if sidx is None else sidx[sel]
            v0, g0 = R.sample_grad(Xs[sel], W, s_ref, params, S, M)
            ev, eg = rel(val[sel], v0), rel(grad[sel], g0)
            print('sample_grad %s T=%d nsamp=%d sidx=%s: val %.2e grad %.2e' % (dtype, T, ns, kind, ev, eg))
            assert ev < VAL_BOUNDS[dtype] and eg < GRAD_BOUNDS[dtype], (ns, kind, ev, eg)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('D,S,M,T', SHAPES)
def test_against_the_cpu_reference(D, S, M, T, dtype):
    eng, params, alpha, Li = _synthetic(D, S, M, dtype)
    _check_against_reference(eng, params, alpha, Li, S, M, synth.make_X(101, T, D), dtype)
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_three_chunks_in_one_call(dtype):
    D, S, M = 5, 4, 60
    eng, params, alpha, Li = _synthetic(D, S, M, dtype)
    _check_against_reference(eng, params, alpha, Li, S, M, synth.make_X(102, 2 * CHUNK + 300, D), dtype, nsamps=(7, 1024))
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('D,S,M,T', SHAPES)
def test_weights_alpha_give_predict_grads_mean_gradient_bit_for_bit(D, S, M, T, dtype):
    eng, params, alpha, Li = _synthetic(D, S, M, dtype)
    Xs = synth.make_X(103, T, D)
    _, _, dmu, _ = eng.predict_grad(Xs, alpha, Li, want_std=False)
    val, grad = eng.sample_grad(Xs, alpha.reshape(-1, 1))
    assert np.array_equal(grad, dmu)
    # Li = 0: every column of W is alpha, so any sidx gives the same bits
    W = eng.sample_weights(alpha, np.zeros_like(Li), 37, seed=5)
    assert np.array_equal(W, np.repeat(alpha.reshape(-1, 1), 37, 1))
    sidx = np.random.default_rng(1).integers(0, 37, T)
    val2, grad2 = eng.sample_grad(Xs, W, sidx=sidx)
    assert np.array_equal(grad2, dmu) and np.array_equal(val2, val)
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_position_independence_bit_for_bit(dtype):
    D, S, M, T, ns = 20, 4, 60, CHUNK + 1500, 23
    eng, params, alpha, Li = _synthetic(D, S, M, dtype)
    Xs = synth.make_X(104, T, D)
    rng = np.random.default_rng(2)
    W = SR.weights(alpha, Li, SR.kappa(params), ns, 4)
    sidx = rng.integers(0, ns, T)
    val, grad = eng.sample_grad(Xs, W, sidx=sidx)
    assert np.array_equal(val, eng.sample_grad(Xs, W, sidx=sidx)[0])                    # the same call twice
    perm = rng.permutation(T)
    vp, gp = eng.sample_grad(Xs[perm], W, sidx=sidx[perm])                               # a permutation permutes the outputs
    assert np.array_equal(vp, val[perm]) and np.array_equal(gp, grad[perm])
    lo, hi = CHUNK - 700, CHUNK + 801                                                    # a slice across the chunk boundary
    vs, gs = eng.sample_grad(Xs[lo:hi], W, sidx=sidx[lo:hi])
    assert np.array_equal(vs, val[lo:hi]) and np.array_equal(gs, grad[lo:hi])
    W2 = np.concatenate((W, rng.standard_normal((W.shape[0], 300))), 1)                  # more columns: nothing changes
    v2, g2 = eng.sample_grad(Xs, W2, sidx=sidx)
    assert np.array_equal(v2, val) and np.array_equal(g2, grad)
    few = rng.choice(ns, 5, replace=False)                                               # unused columns dropped, sidx renumbered
    s5 = rng.integers(0, 5, T)
    va, ga = eng.sample_grad(Xs, W, sidx=few[s5])
    vb, gb = eng.sample_grad(Xs, np.ascontiguousarray(W[:, few]), sidx=s5)
    assert np.array_equal(va, vb) and np.array_equal(ga, gb)
    vn, gn = eng.sample_grad(Xs, W, sidx=sidx, want_val=False)                           # without val: the same grad
    assert vn is None and np.array_equal(gn, grad)
    v0, g0 = eng.sample_grad(Xs, W)                                                      # NULL sidx is t % nsamp
    v1, g1 = eng.sample_grad(Xs, W, sidx=np.arange(T) % ns)
    assert np.array_equal(v0, v1) and np.array_equal(g0, g1)
    eng.close()


def test_f16x3_context_equals_fp32_context():
    from scfgp_amd.engine import HipEngine
    D, S, M, T, ns = 20, 4, 60, CHUNK + 300, 64
    e32, params, alpha, Li = _synthetic(D, S, M, 'f32')
    e16 = HipEngine(D, S, M, dtype='f16x3'); e16.set_params(params)
    Xs = synth.make_X(105, T, D)
    W = SR.weights(alpha, Li, SR.kappa(params), ns, 6)
    sidx = np.random.default_rng(3).integers(0, ns, T)
    a, b = e32.sample_grad(Xs, W, sidx=sidx), e16.sample_grad(Xs, W, sidx=sidx)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    e32.close(); e16.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_values_agree_with_scfgp_sample(dtype):
    D, S, M, T = 5, 4, 60, CHUNK + 500
    eng, params, alpha, Li = _synthetic(D, S, M, dtype)
    Xs = synth.make_X(106, T, D)
    rng = np.random.default_rng(4)
    for ns in (1, 7, 300):
        W = eng.sample_weights(alpha, Li, ns, seed=9)
        sidx = rng.integers(0, ns, T)
        val, _ = eng.sample_grad(Xs, W, sidx=sidx)
        block = eng.sample(Xs, alpha, Li, ns, seed=9)
        e = rel(val, block[np.arange(T), sidx])
        print('sample_grad %s val against scfgp_sample, nsamp=%d: %.2e' % (dtype, ns, e))
        assert e < VAL_BOUNDS[dtype]
    eng.close()


def _scaled_problem(xalgo, yalgo, seed=5, N=600, T=50):
    """test_gpu_predict_grad's problem: an engine trained on scaled data of 4 raw columns, one of them constant"""
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
    return eng, xs, ys, alpha.copy(), Li.copy(), Xr[N:]


NS_SCALED = 16


@pytest.mark.parametrize('xalgo', Scaler.algos)
def test_raw_mode_through_every_x_scaler(xalgo):
    eng, xs, ys, alpha, Li, Xr = _scaled_problem(xalgo, 'normal')
    W = eng.sample_weights(alpha, Li, NS_SCALED, seed=3)
    sidx = np.random.default_rng(6).integers(0, NS_SCALED, Xr.shape[0])
    val, grad = eng.sample_grad(Xr, W, sidx=sidx, mode='raw')
    assert grad.shape == (Xr.shape[0], 4) and np.all(grad[:, 2] == 0)           # the constant column the scaler dropped
    v0, g0 = eng.sample_grad(np.ascontiguousarray(xs.forward_transform(Xr)), W, sidx=sidx)
    cols = xs.data['cols']
    assert rel(val, v0) < 1e-10
    assert rel(grad[:, cols], g0 * G.x_scaler_deriv(xs, Xr)) < 1e-10            # chained by the host derivative
    eng.close()


def _fd_val(f, Xr, cols, h=1e-6):
    """central differences of f (rows -> val (T,)) in the listed raw columns, all rows in one call: tests/test_gpu_predict_grad.py's
    _fd (the same step h max(1, |column|max)) for one output"""
    T, Dr = Xr.shape
    batch = [Xr]
    for c in cols:
        for s in (1, -1):
            Xp = Xr.copy(); Xp[:, c] += s * h * max(1.0, abs(Xr[:, c]).max()); batch.append(Xp)
    v = np.asarray(f(np.vstack(batch))).reshape(-1)
    g = np.zeros((T, Dr))
    for k, c in enumerate(cols):
        hh = 2 * h * max(1.0, abs(Xr[:, c]).max())
        g[:, c] = (v[(1 + 2 * k) * T:(2 + 2 * k) * T] - v[(2 + 2 * k) * T:(3 + 2 * k) * T]) / hh
    return g


@pytest.mark.parametrize('yalgo', Scaler.algos)
def test_y_mode_through_every_y_scaler(yalgo):
    eng, xs, ys, alpha, Li, Xr = _scaled_problem('auto-inv-normal' if yalgo != 'min-max' else 'normal', yalgo)
    T = Xr.shape[0]
    W = eng.sample_weights(alpha, Li, NS_SCALED, seed=8)
    sidx = np.random.default_rng(7).integers(0, NS_SCALED, T)
    val, grad = eng.sample_grad(Xr, W, sidx=sidx, mode='y')
    block = eng.sample(Xr, alpha, Li, NS_SCALED, seed=8, mode='y')[np.arange(T), sidx]
    fin = np.isfinite(block)                                                    # inv-normal scalers: no value outside (0, 1)
    assert np.array_equal(np.isfinite(val), fin) and fin.sum() >= T // 4
    assert rel(val[fin], block[fin]) < VAL_BOUNDS['f64']
    cols = xs.data['cols']
    ncol = 1 + 2 * len(cols)
    fd = _fd_val(lambda X: eng.sample_grad(X, W, sidx=np.tile(sidx, ncol), mode='y')[0], Xr, cols)
    ok = fin & np.isfinite(fd).all(1)
    assert ok.sum() >= T // 4 and np.isfinite(grad[ok]).all()
    e = rel(grad[ok], fd[ok])
    print('sample_grad y mode %s: grad against central differences %.2e' % (yalgo, e))
    assert e < 1e-5                                                             # test_gpu_predict_grad's bound for its raw and y modes
    assert np.array_equal(eng.sample_grad(Xr, W, sidx=sidx, mode='y', want_val=False)[1], grad, equal_nan=True)
    eng.close()


def test_errors_leave_the_outputs_untouched():
    from scfgp_amd.engine import HipEngine
    from scfgp_amd import _lib
    from scfgp_amd._lib import dptr
    D, S, M = 5, 4, 60
    eng, params, alpha, Li = _synthetic(D, S, M, 'f64')
    T, ns = 10, 4
    Xs = synth.make_X(3, T, D)
    W = np.ascontiguousarray(SR.weights(alpha, Li, SR.kappa(params), ns, 1))
    val = np.full(T, -77.0); grad = np.full((T, D), -77.0)
    ip = lambda a: None if a is None else a.ctypes.data_as(_lib._c_i64_p)

    def call(e, Xs=Xs, T=T, W=W, ns=ns, sidx=None, mode=0, val=val, grad=grad):
        rc = e.lib.scfgp_sample_grad(e.ctx, dptr(Xs), T, dptr(W), ns, ip(sidx), mode, dptr(val), dptr(grad))
        assert np.all(val == -77.0) and np.all(grad == -77.0)
        return rc, e.last_error()

    for kw in (dict(Xs=None), dict(W=None), dict(T=0), dict(T=-2), dict(mode=-1), dict(mode=3)):
        rc, msg = call(eng, **kw)
        assert rc == -1 and 'bad arguments' in msg, kw
    assert eng.lib.scfgp_sample_grad(eng.ctx, dptr(Xs), T, dptr(W), ns, None, 0, dptr(val), None) == -1       # grad is required
    assert np.all(val == -77.0)
    for bad in (0, -1, 1025):
        rc, msg = call(eng, ns=bad)
        assert rc == -1 and 'nsamp' in msg
    rc, msg = call(eng, mode=1)
    assert rc == -1 and 'no X scaler' in msg
    sc = Scaler('min-max'); sc.fit(synth.make_X(4, 50, D))
    eng.set_x_scaler(sc)
    rc, msg = call(eng, mode=2)
    assert rc == -1 and 'no y scaler' in msg
    for row, bad in ((7, ns), (2, -1)):                                         # the message names the first bad row
        sidx = np.zeros(T, dtype=np.int64); sidx[row] = bad; sidx[9] = ns + 5
        rc, msg = call(eng, sidx=sidx)
        assert rc == -1 and 'row %d' % row in msg and str(bad) in msg, msg
    with pytest.raises(ValueError, match='row 7'):
        s = np.zeros(T, dtype=np.int64); s[7] = ns
        eng.sample_grad(Xs, W, sidx=s)
    for bad in (np.nan, np.inf, -np.inf):
        Wb = W.copy(); Wb[3, 2] = bad
        rc, msg = call(eng, W=Wb)
        assert rc == -4 and 'non-finite' in msg
        with pytest.raises(FloatingPointError):
            eng.sample_grad(Xs, Wb)
    Xn = Xs.copy(); Xn[4, 1] = np.nan                                            # a non-finite row: non-finite outputs, no error
    v, g = eng.sample_grad(Xn, W)
    assert not np.isfinite(v[4]) and not np.isfinite(g[4]).any()
    ok = np.arange(T) != 4
    v0, g0 = eng.sample_grad(Xs, W)
    assert np.array_equal(v[ok], v0[ok]) and np.array_equal(g[ok], g0[ok])
    with pytest.raises(ValueError):
        eng.sample_grad(Xs, W, mode='bogus')
    with pytest.raises(ValueError):
        eng.sample_grad(Xs, W[:-1])
    with pytest.raises(ValueError):
        eng.sample_grad(Xs, W, sidx=np.zeros(T + 1, dtype=np.int64))
    eng.close()
    fresh = HipEngine(D, S, M, dtype='f64')                                      # no parameters yet
    rc, msg = call(fresh)
    assert rc == -1 and 'parameters not set' in msg
    fresh.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_training_state_survives(dtype):
    from scfgp_amd.engine import HipEngine
    D, S, M = 20, 4, 60
    params = synth.make_params(7, D, S, M, abc=(-1.0, 0.0, -1.0))
    X = synth.make_X(7, 1500, D)
    y = np.sin(3 * X[:, :1]) + 0.1 * synth.normal(10, 0, 1500)[:, None]
    eng = HipEngine(D, S, M, dtype=dtype); eng.set_params(params); eng.set_data(X, y)
    c0, g0, a0, L0 = eng.eval(want_grad=True)
    c0, g0, a0, L0 = float(c0), g0.copy(), a0.copy(), L0.copy()
    Xs = synth.make_X(9, CHUNK + 200, D)
    eng.sample_grad(Xs, eng.sample_weights(a0, L0, 40, seed=2), sidx=None)
    c1, g1, a1, L1 = eng.eval(want_grad=True)
    assert float(c1) == c0 and np.array_equal(g1, g0) and np.array_equal(a1, a0) and np.array_equal(L1, L0)
    eng.close()


def test_facade_sample_maximize():
    from scfgp_amd import SCFGP
    rng = np.random.default_rng(5)
    np.random.seed(5)
    X = rng.uniform(-2, 2, (300, 2))
    y = np.sin(2 * X[:, :1]) * np.cos(X[:, 1:2]) + 0.05 * rng.standard_normal((300, 1))
    model = SCFGP(sparsity=2, nfeats=12, device_scaler=True)                     # an fp64 context
    model.set_data(X[:240], y[:240])
    model.optimize(X[240:], y[240:], max_iter=20,
                   algo={'algo': 'adam', 'algo_params': {'learning_rate': 0.02, 'beta1': 0.9, 'beta2': 0.999, 'epsilon': 1e-8}})
    a0, L0 = model.alpha.copy(), model.Li.copy()
    g = np.linspace(-2.0, 2.0, 12)
    pool = np.stack(np.meshgrid(g, g, indexing='ij'), -1).reshape(-1, 2)
    ns, gtol = 16, 1e-6
    owner = model.pred_func.__self__
    eng = owner.engine
    params = model.params.get_value()
    sidx = np.arange(ns)
    for minimize in (False, True):
        Xb, val_y, start, conv = model.sample_maximize(pool, ns, seed=3, minimize=minimize, gtol=gtol)
        assert Xb.shape == (ns, 2) and val_y.shape == (ns,) and conv.shape == (ns,) and conv.dtype == bool
        assert np.array_equal(start, model.sample_argmax(pool, ns, seed=3, minimize=minimize)[0])
        W = eng.sample_weights(model.alpha, model.Li, ns, seed=3)
        v_start, _ = eng.sample_grad(pool[start], W, sidx=sidx, mode='raw')
        v_best, _ = eng.sample_grad(Xb, W, sidx=sidx, mode='raw')
        assert np.all(v_best <= v_start) if minimize else np.all(v_best >= v_start)
        assert np.all(Xb >= pool.min(0)) and np.all(Xb <= pool.max(0))
        block = model.sample(Xb, ns, seed=3)                                     # mode 'y', no noise
        assert rel(val_y, block[sidx, sidx]) < VAL_BOUNDS['f64']
        # rows flagged converged are stationary by the numpy reference, in raw X: the scaled closed form chained through the X scaler.
        # The reference's gradient differs from the device's by the fp64 parity bound, 1e-10 of gradients of order 1: slack 1e-8
        vr, gr = R.sample_grad(model.X_scaler.forward_transform(Xb), W, sidx, params, model.S, model.M)
        gr = gr * G.x_scaler_deriv(model.X_scaler, Xb)
        pg = R.projected_gradient_norm(Xb, gr, pool.min(0), pool.max(0), minimize=minimize)
        assert np.all(pg[conv] <= gtol * np.maximum(1.0, np.abs(vr[conv])) + 1e-8)
        print('sample_maximize minimize=%s: %d of %d converged' % (minimize, conv.sum(), ns))
    lo, hi = np.array([-1.0, -0.5]), np.array([0.5, 1.0])                        # explicit bounds: starts must lie inside them
    inside = pool[((pool >= lo) & (pool <= hi)).all(1)]
    Xb, _, _, _ = model.sample_maximize(inside, ns, seed=3, bounds=(lo, hi))
    assert np.all(Xb >= lo) and np.all(Xb <= hi)
    assert np.array_equal(model.alpha, a0) and np.array_equal(model.Li, L0)      # nothing of the model is touched
    other = SCFGP(sparsity=2, nfeats=12)
    other.pred_func = lambda Xs, alpha, Li: None
    with pytest.raises(TypeError):
        other.sample_maximize(pool, 4)
