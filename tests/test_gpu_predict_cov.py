"""GPU tier of the joint posterior covariance (predcov.hip: scfgp_predict_cov): parity with the numpy closed form
(tests/pred_cov_ref.py) in the symmetric and the cross form, consistency with predict's variance and with the observation noise, the
bit-level guarantees (symmetry, symmetric = cross, blocks of a large call = the calls on the subsets, f16x3 = fp32, repeatability), the
sample covariance of scfgp_sample's draws, the input modes, the SCFGP.predict_cov facade, survival of the training state and the
argument errors."""
import numpy as np
import pytest

from scfgp_amd import synth
from scfgp_amd.scaler import Scaler
from tests import pred_cov_ref as R

pytestmark = pytest.mark.gpu


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


# (D, S, M, Ta, Tb): K = 128, 600, 2112, a small odd J, rank-S projection at small K; no T is a multiple of 16 or of the 128-wide tile
SHAPES = [(5, 4, 60, 391, 203), (20, 20, 280, 1001, 333), (64, 32, 1024, 777, 389), (3, 1, 20, 301, 157), (40, 4, 100, 519, 1100)]
# fp64: the bound tests/test_gpu_sample.py and tests/test_gpu_predict_grad.py use for this class of product.  fp32: twice
# test_gpu_sample.py's BOUNDS['f32'] = 3e-6 -- the covariance is bilinear in two fp32 factors each of which that test bounds at 3e-6.
BOUNDS = {'f64': 1e-10, 'f32': 6e-6}


def _synthetic(D, S, M, dtype):
    """an engine with parameters set and the synthetic Li of tests/test_gpu_sample.py"""
    from scfgp_amd.engine import HipEngine
    seed = 0x5CF65000 + M
    K = 2 * (S + M)
    params = synth.make_params(seed + 0x0202, D, S, M, abc=(-1.0, 0.0, -1.0))
    rng = np.random.default_rng(seed)
    alpha = rng.standard_normal(K) / np.sqrt(K)
    Li = np.tril(rng.standard_normal((K, K))) / np.sqrt(K)
    eng = HipEngine(D, S, M, dtype=dtype); eng.set_params(params)
    return eng, params, alpha, Li


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('D,S,M,Ta,Tb', SHAPES)
def test_parity_symmetric_and_cross(D, S, M, Ta, Tb, dtype):
    eng, params, alpha, Li = _synthetic(D, S, M, dtype)
    Xa = synth.make_X(101, Ta, D); Xb = synth.make_X(202, Tb, D)
    sym = eng.predict_cov(Xa, Li)
    assert sym.shape == (Ta, Ta) and sym.dtype == np.float64
    e = rel(sym, R.pred_cov(Xa, Li, params, S, M))
    print('parity symmetric', (D, S, M, Ta), dtype, e)
    assert e < BOUNDS[dtype], e
    cross = eng.predict_cov(Xa, Li, Xb=Xb)
    assert cross.shape == (Ta, Tb)
    e = rel(cross, R.pred_cov(Xa, Li, params, S, M, Xb=Xb))
    print('parity cross', (D, S, M, Ta, Tb), dtype, e)
    assert e < BOUNDS[dtype], e
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_parity_across_chunks_and_panels(dtype):
    """Ta = 70 001 rows (three upload chunks) against 33 columns: rows at both ends, in the middle and around the chunk boundary"""
    D, S, M, Ta, Tb = 64, 32, 1024, 70001, 33
    eng, params, alpha, Li = _synthetic(D, S, M, dtype)
    Xa = synth.make_X(101, Ta, D); Xb = synth.make_X(202, Tb, D)
    cov = eng.predict_cov(Xa, Li, Xb=Xb)
    assert cov.shape == (Ta, Tb)
    sel = np.unique(np.r_[0:40, Ta // 2:Ta // 2 + 40, 32760:32800, 65530:65560, Ta - 40:Ta])
    e = rel(cov[sel], R.pred_cov(Xa[sel], Li, params, S, M, Xb=Xb))
    print('parity chunks', dtype, e)
    assert e < BOUNDS[dtype], e
    assert np.all(np.isfinite(cov))
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('D,S,M', [(5, 4, 60), (64, 32, 1024)])
def test_diagonal_is_predicts_variance_and_noise_adds_kappa(D, S, M, dtype):
    eng, params, alpha, Li = _synthetic(D, S, M, dtype)
    Xs = synth.make_X(7, 333, D)
    kap = R.kappa(params)
    _, sd = eng.predict(Xs, alpha, Li)
    cov = eng.predict_cov(Xs, Li)
    e = float(np.max(np.abs(np.diag(cov) + kap - sd ** 2) / sd ** 2))
    print('diagonal against predict', (D, S, M), dtype, e)
    assert e < BOUNDS[dtype], e
    noisy = eng.predict_cov(Xs, Li, noise=True)
    # exactly kappa on the diagonal and nothing elsewhere; the device forms kappa = log(1 + e^c) itself: the host's value or a neighbour
    off = ~np.eye(333, dtype=bool)
    assert np.array_equal(noisy[off], cov[off])
    assert any(np.array_equal(np.diag(noisy), np.diag(cov) + k) for k in (kap, np.nextafter(kap, 0.0), np.nextafter(kap, 1e9)))
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_bit_level_guarantees(dtype):
    D, S, M = 20, 20, 280
    eng, params, alpha, Li = _synthetic(D, S, M, dtype)
    X = synth.make_X(55, 2500, D)
    cov = eng.predict_cov(X, Li)
    assert np.array_equal(cov, cov.T)
    assert np.array_equal(cov, eng.predict_cov(X, Li))                              # two calls agree
    assert np.array_equal(cov, eng.predict_cov(X, Li, Xb=X))                        # symmetric = cross on the same rows
    # blocks: row / column subsets that straddle tile boundaries (multiples of 128)
    for (r0, r1), (c0, c1) in (((100, 300), (1000, 1301)), ((0, 2500), (120, 140)), ((2390, 2500), (0, 2500)), ((255, 257), (383, 386))):
        assert np.array_equal(cov[r0:r1, c0:c1], eng.predict_cov(X[r0:r1], Li, Xb=X[c0:c1]))
    assert np.array_equal(cov[700:1500, 700:1500], eng.predict_cov(X[700:1500], Li))
    # panels: 9000 columns make a staging panel 1792 rows high, so 2500 rows leave in two panels
    Xw = synth.make_X(56, 9000, D)
    wide = eng.predict_cov(X, Li, Xb=Xw)
    assert np.array_equal(wide[1700:1900, 4000:4300], eng.predict_cov(X[1700:1900], Li, Xb=Xw[4000:4300]))
    assert np.array_equal(wide[:, :2500].T, eng.predict_cov(Xw[:2500], Li, Xb=X))
    del wide
    # chunks: 33 000 rows cross the chunk boundary at 32 768
    Xl = synth.make_X(57, 33000, D)
    tall = eng.predict_cov(Xl, Li, Xb=X[:50])
    assert np.array_equal(tall[32700:32900], eng.predict_cov(Xl[32700:32900], Li, Xb=X[:50]))
    assert np.array_equal(tall[32768:], eng.predict_cov(Xl[32768:], Li, Xb=X[:50]))
    assert np.array_equal(tall[100:200, 10:20], eng.predict_cov(Xl[100:200], Li, Xb=X[10:20]))
    eng.close()


def test_f16x3_context_equals_fp32_context():
    from scfgp_amd.engine import HipEngine
    D, S, M = 64, 32, 1024
    e32, params, alpha, Li = _synthetic(D, S, M, 'f32')
    e16 = HipEngine(D, S, M, dtype='f16x3'); e16.set_params(params)
    Xa = synth.make_X(202, 1500, D); Xb = synth.make_X(203, 301, D)
    assert np.array_equal(e32.predict_cov(Xa, Li, noise=True), e16.predict_cov(Xa, Li, noise=True))
    assert np.array_equal(e32.predict_cov(Xa, Li, Xb=Xb), e16.predict_cov(Xa, Li, Xb=Xb))
    e32.close(); e16.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_sample_covariance_of_the_device_draws(dtype):
    """the covariance of 1024 draws of scfgp_sample at 64 points, element-wise within 5 CLT standard errors of predict_cov (standard
    error of a Gaussian sample covariance: sqrt((c_ii c_jj + c_ij^2) / (n - 1))), the margin test_gpu_sample.py gives the moments"""
    from scfgp_amd.engine import HipEngine
    D, S, M = 4, 3, 40
    params = synth.make_params(17, D, S, M, abc=(-1.0, 0.0, -1.0))
    X = synth.make_X(17, 800, D)
    y = np.sin(3 * X[:, :1]) + 0.1 * synth.normal(20, 0, 800)[:, None]
    eng = HipEngine(D, S, M, dtype=dtype); eng.set_params(params); eng.set_data(X, y)
    _, _, alpha, Li = eng.eval(want_grad=False)
    Xs = synth.make_X(18, 64, D)
    ns = 1024
    f = eng.sample(Xs, alpha, Li, ns, seed=31)
    cov = eng.predict_cov(Xs, Li)
    d = np.diag(cov)
    se = np.sqrt((np.outer(d, d) + cov ** 2) / (ns - 1))
    z = float(np.max(np.abs(np.cov(f) - cov) / se))
    print('sample covariance, worst z', dtype, z)
    assert z < 5
    eng.close()


def _scaled_problem(xalgo, yalgo, seed=5, N=600, T=50):
    """test_gpu_sample's problem: an engine trained on scaled data of 4 raw columns, one of them constant"""
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
    Xa, Xb = Xr[:30], Xr[20:]
    fa, fb = (np.ascontiguousarray(xs.forward_transform(x)) for x in (Xa, Xb))
    assert Xa.shape[1] == 4 and fa.shape[1] == 3                                    # the constant column is dropped
    for noise in (False, True):
        assert rel(eng.predict_cov(Xa, Li, mode='raw', noise=noise), eng.predict_cov(fa, Li, noise=noise)) < 1e-12
    assert rel(eng.predict_cov(Xa, Li, Xb=Xb, mode='raw'), eng.predict_cov(fa, Li, Xb=fb)) < 1e-12
    eng.close()


def test_facade_predict_cov():
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
    Xs, Xs2 = X[240:], X[250:270]
    cov = model.predict_cov(Xs, noise=True)
    assert cov.shape == (60, 60) and np.array_equal(cov, cov.T)
    eng = model.pred_func.__self__.engine
    assert np.array_equal(cov, eng.predict_cov(Xs, model.Li, mode='raw', noise=True))
    cross = model.predict_cov(Xs, Xs2)
    assert cross.shape == (60, 20)
    assert np.array_equal(cross, eng.predict_cov(Xs, model.Li, Xb=Xs2, mode='raw'))
    assert np.array_equal(cross, model.predict_cov(Xs)[:, 10:30])
    # the diagonal with noise is the squared std of the scaled target that pred_func reports
    _, sd = model.pred_func(np.ascontiguousarray(model.X_scaler.forward_transform(Xs), dtype=np.float64), model.alpha, model.Li)
    assert np.max(np.abs(np.diag(cov) - sd ** 2) / sd ** 2) < 1e-10
    other = SCFGP(sparsity=3, nfeats=12)
    other.pred_func = lambda Xs, alpha, Li: None
    with pytest.raises(TypeError):
        other.predict_cov(Xs)


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
    eng.predict_cov(Xs, L0, Xb=Xs[:100])
    eng.predict_cov(Xs[:700], L0, noise=True)
    c1, g1, a1, L1 = eng.eval(want_grad=True)
    assert float(c1) == c0 and np.array_equal(g1, g0) and np.array_equal(a1, a0) and np.array_equal(L1, L0)
    for u, v in zip(eng.predict(Xs, a0, L0), p0):
        assert np.array_equal(u, v)
    for u, v in zip(eng.predict_grad(Xs[:3000], a0, L0), q0):           # shares its factor buffers with predict_cov
        assert np.array_equal(u, v)
    eng.close()


def test_errors():
    from scfgp_amd.engine import HipEngine
    from scfgp_amd._lib import dptr
    eng, params, alpha, Li = _synthetic(5, 4, 60, 'f64')
    Xs = synth.make_X(3, 10, 5)
    with pytest.raises(ValueError, match='Ta'):
        eng.predict_cov(Xs[:0], Li)                                       # Ta = 0
    with pytest.raises(ValueError):
        eng.predict_cov(Xs, Li, Xb=Xs[:0])                                # Tb = 0
    with pytest.raises(ValueError, match='Tb'):
        eng.predict_cov(Xs, Li, Xb=np.zeros((32769, 5)))                  # Tb = 32 769
    with pytest.raises(ValueError, match='32768'):
        eng.predict_cov(np.zeros((32769, 5)), Li)                         # the symmetric form's Tb is Ta
    with pytest.raises(ValueError, match='columns'):
        eng.predict_cov(Xs[:, :4], Li)
    with pytest.raises(ValueError, match='columns'):
        eng.predict_cov(Xs, Li, Xb=Xs[:, :3])
    with pytest.raises(ValueError, match='shape'):
        eng.predict_cov(Xs, Li[:-1])
    with pytest.raises(ValueError, match='noise'):
        eng.predict_cov(Xs, Li, Xb=Xs, noise=True)
    with pytest.raises(ValueError):
        eng.predict_cov(Xs, Li, mode='y')                                 # no raw-y covariance
    with pytest.raises(ValueError, match='scaler'):
        eng.predict_cov(Xs, Li, mode='raw')
    out = np.empty((10, 10))

    def lib_cov(Tb, mode):                                               # past the engine's own checks: the library's messages
        eng._check(eng.lib.scfgp_predict_cov(eng.ctx, dptr(Xs), 10, dptr(Xs), Tb, dptr(Li), mode, 0, dptr(out)), 'predict_cov')
    with pytest.raises(ValueError, match='Tb'):
        lib_cov(0, 0)
    with pytest.raises(ValueError, match='no X scaler'):
        lib_cov(10, 1)
    ok = eng.predict_cov(Xs, Li)                                          # the context still works
    assert rel(ok, R.pred_cov(Xs, Li, params, 4, 60)) < 1e-10
    eng.close()
    fresh = HipEngine(5, 4, 60, dtype='f64')                             # no parameters yet
    with pytest.raises(ValueError, match='parameters not set'):
        fresh.predict_cov(Xs, Li)
    fresh.close()
