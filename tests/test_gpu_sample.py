"""GPU tier of the posterior sample functions (sample.hip: scfgp_sample_weights, scfgp_sample): weights and samples against the numpy
restatement of the generator (tests/sample_ref.py), bit-level consistency across calls, rows, chunks and sample counts, the posterior
moments on the device, the three input modes, the f16x3 context, survival of the training state, the SCFGP.sample facade and the
argument errors."""
import numpy as np
import pytest

from scfgp_amd import synth
from scfgp_amd.scaler import Scaler
from tests import sample_ref as R

pytestmark = pytest.mark.gpu


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


# those of tests/test_gpu_predict_grad.py: K = 128, 600, 2112 over three upload chunks (rank-S projection), a small odd J, rank-S at small K
SHAPES = [(5, 4, 60, 3001), (20, 20, 280, 5000), (64, 32, 1024, 70001), (3, 1, 20, 700), (40, 4, 100, 2000)]
BOUNDS = {'f64': 1e-10, 'f32': 3e-6}


def _synthetic(D, S, M, dtype):
    """an engine with parameters set and the synthetic alpha / Li of test_gpu_round2's predict test"""
    from scfgp_amd.engine import HipEngine
    seed = 0x5CF65000 + M
    K = 2 * (S + M)
    params = synth.make_params(seed + 0x0202, D, S, M, abc=(-1.0, 0.0, -1.0))
    rng = np.random.default_rng(seed)
    alpha = rng.standard_normal(K) / np.sqrt(K)
    Li = np.tril(rng.standard_normal((K, K))) / np.sqrt(K)
    eng = HipEngine(D, S, M, dtype=dtype); eng.set_params(params)
    return eng, params, alpha, Li


@pytest.mark.parametrize('dtype', ['f64', 'f32', 'f16x3'])
@pytest.mark.parametrize('D,S,M', [(5, 4, 60), (64, 32, 1024)])
def test_weights_against_the_cpu(D, S, M, dtype):
    eng, params, alpha, Li = _synthetic(D, S, M, dtype)
    for ns in (1, 7, 300):
        W = eng.sample_weights(alpha, Li, ns, seed=123)
        assert W.shape == (2 * (S + M), ns)
        assert rel(W, R.weights(alpha, Li, R.kappa(params), ns, 123)) < 1e-12
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('D,S,M,T', SHAPES)
def test_samples_against_the_cpu(D, S, M, T, dtype):
    eng, params, alpha, Li = _synthetic(D, S, M, dtype)
    Xs = synth.make_X(101, T, D)
    sel = np.unique(np.r_[0:40, T // 2:T // 2 + 40, 32760:32800, T - 40:T] % T)
    for ns, noise in ((1, False), (7, True), (64, False), (300, True)):
        out = eng.sample(Xs, alpha, Li, ns, seed=9, noise=noise)
        assert out.shape == (T, ns)
        ref = R.samples(Xs[sel], alpha, Li, params, S, M, ns, 9)
        if noise:
            ref = ref + np.sqrt(R.kappa(params)) * R.normals(sel, ns, 9, 1)
        e = rel(out[sel], ref)
        assert e < BOUNDS[dtype], (ns, noise, e)
    eng.close()


def test_consistency_bit_for_bit():
    eng, params, alpha, Li = _synthetic(20, 20, 280, 'f32')
    T = 40000
    Xs = synth.make_X(55, T, 20)
    a = eng.sample(Xs, alpha, Li, 8, seed=4)
    assert np.array_equal(a, eng.sample(Xs, alpha, Li, 8, seed=4))                      # same seed twice
    lo, hi = 32000, 33500                                                                # across the chunk boundary 32768
    assert np.array_equal(a[lo:hi], eng.sample(Xs[lo:hi], alpha, Li, 8, seed=4))        # rows do not matter without noise
    yn = eng.sample(Xs, alpha, Li, 8, seed=4, noise=True)
    assert np.array_equal(eng.sample(Xs[:33000], alpha, Li, 8, seed=4, noise=True), yn[:33000])
    assert np.array_equal(a[:, :5], eng.sample(Xs, alpha, Li, 5, seed=4))                # sample s does not depend on nsamp
    assert np.array_equal(a[:, :5], eng.sample(Xs, alpha, Li, 300, seed=4)[:, :5])
    assert not np.any(a == eng.sample(Xs, alpha, Li, 8, seed=5))                         # another seed, other functions
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_moments_on_the_device(dtype):
    from scfgp_amd.engine import HipEngine
    D, S, M = 4, 3, 40
    params = synth.make_params(17, D, S, M, abc=(-1.0, 0.0, -1.0))
    X = synth.make_X(17, 800, D)
    y = np.sin(3 * X[:, :1]) + 0.1 * synth.normal(20, 0, 800)[:, None]
    eng = HipEngine(D, S, M, dtype=dtype); eng.set_params(params); eng.set_data(X, y)
    _, _, alpha, Li = eng.eval(want_grad=False)
    Xs = synth.make_X(18, 64, D)
    mu, sd = eng.predict(Xs, alpha, Li)
    kap = R.kappa(params)
    ns = 1024
    f = eng.sample(Xs, alpha, Li, ns, seed=31)
    var_f = sd ** 2 - kap
    assert np.max(np.abs(f.mean(1) - mu.ravel()) / np.sqrt(var_f / ns)) < 5
    assert np.max(np.abs(f.var(1, ddof=1) - var_f) / (var_f * np.sqrt(2 / (ns - 1)))) < 5
    yv = eng.sample(Xs, alpha, Li, ns, seed=31, noise=True)
    assert np.max(np.abs(yv.mean(1) - mu.ravel()) / (sd / np.sqrt(ns))) < 5
    assert np.max(np.abs(yv.var(1, ddof=1) - sd ** 2) / (sd ** 2 * np.sqrt(2 / (ns - 1)))) < 5
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


@pytest.mark.parametrize('xalgo', Scaler.algos)
def test_raw_mode_equals_scaled_mode(xalgo):
    eng, xs, ys, alpha, Li, Xr = _scaled_problem(xalgo, 'normal')
    for noise in (False, True):
        a = eng.sample(Xr, alpha, Li, 16, seed=3, mode='raw', noise=noise)
        b = eng.sample(np.ascontiguousarray(xs.forward_transform(Xr)), alpha, Li, 16, seed=3, noise=noise)
        assert rel(a, b) < 1e-12
    eng.close()


@pytest.mark.parametrize('yalgo', Scaler.algos)
def test_y_mode_through_every_y_scaler(yalgo):
    eng, xs, ys, alpha, Li, Xr = _scaled_problem('auto-inv-normal' if yalgo != 'min-max' else 'normal', yalgo)
    for noise in (False, True):
        f = eng.sample(Xr, alpha, Li, 16, seed=8, mode='raw', noise=noise)
        y = eng.sample(Xr, alpha, Li, 16, seed=8, mode='y', noise=noise)
        ref = ys.backward_transform(f.reshape(-1, 1)).reshape(f.shape)
        fin = np.isfinite(ref)
        assert np.array_equal(np.isfinite(y), fin)                    # inv-normal scalers: no value outside (0, 1), as predict_y
        assert fin.sum() >= fin.size // 4
        assert rel(y[fin], ref[fin]) < 1e-12
    eng.close()


def test_f16x3_context_equals_fp32_context():
    D, S, M, T = 64, 32, 1024, 40000
    e32, params, alpha, Li = _synthetic(D, S, M, 'f32')
    from scfgp_amd.engine import HipEngine
    e16 = HipEngine(D, S, M, dtype='f16x3'); e16.set_params(params)
    Xs = synth.make_X(202, T, D)
    for ns, noise in ((64, False), (300, True)):
        assert np.array_equal(e32.sample(Xs, alpha, Li, ns, seed=1, noise=noise), e16.sample(Xs, alpha, Li, ns, seed=1, noise=noise))
    assert np.array_equal(e32.sample_weights(alpha, Li, 33, 6), e16.sample_weights(alpha, Li, 33, 6))
    e32.close(); e16.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_training_state_survives(dtype):
    from scfgp_amd.engine import HipEngine
    D, S, M = 20, 20, 280
    params = synth.make_params(7, D, S, M, abc=(-1.0, 0.0, -1.0))
    X = synth.make_X(7, 1500, D)
    y = np.sin(3 * X[:, :1]) + 0.1 * synth.normal(10, 0, 1500)[:, None]
    eng = HipEngine(D, S, M, dtype=dtype); eng.set_params(params); eng.set_data(X, y)
    c0, g0, a0, L0 = eng.eval(want_grad=True)
    c0, g0, a0, L0 = float(c0), g0.copy(), a0.copy(), L0.copy()
    Xs = synth.make_X(9, 33000, D)
    p0 = eng.predict(Xs, a0, L0)
    q0 = eng.predict_grad(Xs[:3000], a0, L0)
    eng.sample(Xs, a0, L0, 40, seed=2, noise=True)
    eng.sample_weights(a0, L0, 40, seed=2)
    c1, g1, a1, L1 = eng.eval(want_grad=True)
    assert float(c1) == c0 and np.array_equal(g1, g0) and np.array_equal(a1, a0) and np.array_equal(L1, L0)
    for u, v in zip(eng.predict(Xs, a0, L0), p0):
        assert np.array_equal(u, v)
    for u, v in zip(eng.predict_grad(Xs[:3000], a0, L0), q0):
        assert np.array_equal(u, v)
    eng.close()


def test_facade_sample():
    from scfgp_amd import SCFGP
    rng = np.random.default_rng(5)
    np.random.seed(5)
    X = rng.uniform(-2, 2, (300, 3))
    X = np.column_stack([X[:, :2], np.full(300, 4.0), X[:, 2:]])     # a constant column
    y = np.sin(X[:, :1]) + 0.5 * X[:, 1:2] ** 2 + 0.05 * rng.standard_normal((300, 1))
    model = SCFGP(sparsity=3, nfeats=12, device_scaler=True)
    model.set_data(X[:240], y[:240])
    model.optimize(X[240:], y[240:], max_iter=20,
                   algo={'algo': 'adam', 'algo_params': {'learning_rate': 0.02, 'beta1': 0.9, 'beta2': 0.999, 'epsilon': 1e-8}})
    Xs = X[240:]
    s = model.sample(Xs, 12, seed=3, noise=True)
    assert s.shape == (60, 12)
    eng = model.pred_func.__self__.engine
    assert np.array_equal(s, eng.sample(Xs, model.alpha, model.Li, 12, seed=3, mode='y', noise=True))
    other = SCFGP(sparsity=3, nfeats=12)
    other.pred_func = lambda Xs, alpha, Li: None
    with pytest.raises(TypeError):
        other.sample(Xs, 4)


def test_errors():
    from scfgp_amd.engine import HipEngine
    from scfgp_amd._lib import dptr
    eng, params, alpha, Li = _synthetic(5, 4, 60, 'f64')
    Xs = synth.make_X(3, 10, 5)
    for ns in (0, 1025):
        with pytest.raises(ValueError, match='nsamp'):
            eng.sample(Xs, alpha, Li, ns)
        with pytest.raises(ValueError, match='nsamp'):
            eng.sample_weights(alpha, Li, ns)
    with pytest.raises(ValueError, match='bad arguments'):
        eng.sample(Xs[:0], alpha, Li, 4)                                  # T < 1
    with pytest.raises(ValueError):
        eng.sample(Xs, alpha, Li, 4, mode='bogus')
    out = np.empty((10, 4))

    def lib_sample(mode):                                                # past the engine's own checks: the library's messages
        eng._check(eng.lib.scfgp_sample(eng.ctx, dptr(Xs), 10, dptr(alpha), dptr(Li), 4, 0, mode, 0, dptr(out)), 'sample')
    with pytest.raises(ValueError, match='no X scaler'):
        lib_sample(1)
    sc = Scaler('min-max'); sc.fit(synth.make_X(4, 50, 5))
    eng.set_x_scaler(sc)
    with pytest.raises(ValueError, match='no y scaler'):
        lib_sample(2)
    eng.close()
    fresh = HipEngine(5, 4, 60, dtype='f64')                             # no parameters yet
    with pytest.raises(ValueError, match='parameters not set'):
        fresh.sample(Xs, alpha, Li, 4)
    with pytest.raises(ValueError, match='parameters not set'):
        fresh.sample_weights(alpha, Li, 4)
    fresh.close()
