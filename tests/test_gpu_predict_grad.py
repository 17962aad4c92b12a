"""GPU tier of scfgp_predict_grad (predgrad.hip): input gradients of the predictive mean and std against the fp64 CPU reference
(tests/pred_grad_ref.py), bit-equality of mu / std with the predict family, the scalers' chain rules against finite differences, the
f16x3 context, survival of the training state, and the SCFGP.predict_grad facade."""
import numpy as np
import pytest

from oracle import scfgp_oracle as O
from scfgp_amd import synth
from scfgp_amd.scaler import Scaler
from tests import pred_grad_ref as R

pytestmark = pytest.mark.gpu


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def _engine(D, S, M, dtype, N=1500, seed=7):
    from scfgp_amd.engine import HipEngine
    params = synth.make_params(seed, D, S, M, abc=(-1.0, 0.0, -1.0))
    X = synth.make_X(seed, N, D)
    y = np.sin(3 * X[:, :1]) + 0.1 * synth.normal(seed + 3, 0, N)[:, None]
    eng = HipEngine(D, S, M, dtype=dtype)
    eng.nonfinite = 'return'                 # S = 1: the penalty's log of a zero spread makes the cost -inf; alpha and Li are fine
    eng.set_params(params); eng.set_data(X, y)
    _, _, alpha, Li = eng.eval(want_grad=False)
    return eng, params, alpha.copy(), Li.copy()


# (D, S, M, T): K = 128 (64-wide tiles only), K = 600, K = 2112 over three upload chunks (T not a multiple of 256; Sp < Dp: the
# feature map takes the rank-S projection), a small odd J, and the rank-S projection at a small K
SHAPES = [(5, 4, 60, 3001), (20, 20, 280, 5000), (64, 32, 1024, 70001), (3, 1, 20, 700), (40, 4, 100, 2000)]
BOUNDS = {'f64': (1e-10, 1e-10), 'f32': (3e-5, 3e-4)}


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('D,S,M,T', SHAPES)
def test_against_the_cpu_reference(D, S, M, T, dtype):
    eng, params, alpha, Li = _engine(D, S, M, dtype)
    Xs = synth.make_X(101, T, D)
    mu, sd, dmu, dsd = eng.predict_grad(Xs, alpha, Li)
    assert mu.shape == (T, 1) and sd.shape == (T,) and dmu.shape == (T, D) and dsd.shape == (T, D)
    mu_p, sd_p = eng.predict(Xs, alpha, Li)
    assert np.array_equal(mu, mu_p) and np.array_equal(sd, sd_p)
    sel = np.unique(np.r_[0:40, T // 2:T // 2 + 40, 32760:32800, T - 40:T] % T)
    _, _, gmu, gsd = R.predict_grad(Xs[sel], alpha, Li, params, S, M)
    bmu, bsd = BOUNDS[dtype]
    e_mu, e_sd = rel(dmu[sel], gmu), rel(dsd[sel], gsd)
    assert e_mu < bmu and e_sd < bsd, (e_mu, e_sd)
    mu1, sd1, dmu1, dsd1 = eng.predict_grad(Xs, alpha, Li, want_std=False)     # no V* product: the same mean gradient
    assert dsd1 is None and np.array_equal(dmu1, dmu) and np.array_equal(mu1, mu) and np.array_equal(sd1, sd)
    eng.close()


def _scaled_problem(xalgo, yalgo, seed=5, N=600, T=50):
    """An engine trained on scaled data of 4 raw columns, one of them constant (dropped by the X scaler)."""
    from scfgp_amd.engine import HipEngine
    rng = np.random.default_rng(seed)
    Xr = np.column_stack([rng.uniform(0.5, 3.0, N + T), rng.gamma(2.0, 1.0, N + T), np.full(N + T, 2.5), rng.normal(1.0, 2.0, N + T)])
    yr = np.exp(0.3 * np.sin(Xr[:, :1]) + 0.1 * Xr[:, 1:2]) + 0.05 * rng.standard_normal((N + T, 1))
    xs = Scaler(xalgo); xs.fit(Xr[:N]); ys = Scaler(yalgo); ys.fit(yr[:N])
    D, S, M = 3, 2, 40
    eng = HipEngine(D, S, M, dtype='f64')
    eng.set_params(synth.make_params(seed, D, S, M, abc=(-1.0, 0.0, -4.0)))     # small noise: mu +- std stays inside (0, 1) mostly
    eng.set_data(np.ascontiguousarray(xs.forward_transform(Xr[:N])), np.ascontiguousarray(ys.forward_transform(yr[:N])))
    _, _, alpha, Li = eng.eval(want_grad=False)
    eng.set_x_scaler(xs); eng.set_y_scaler(ys)
    return eng, xs, ys, alpha.copy(), Li.copy(), Xr[N:]


def _fd(f, Xr, cols, h=1e-6):
    """central differences of f (rows -> (mu (T,1), sd)) in the listed raw columns, all rows in one call"""
    T, Dr = Xr.shape
    batch = [Xr]
    for c in cols:
        for s in (1, -1):
            Xp = Xr.copy(); Xp[:, c] += s * h * max(1.0, abs(Xr[:, c]).max()); batch.append(Xp)
    mu, sd = f(np.vstack(batch))
    mu = np.asarray(mu).reshape(-1); sd = np.asarray(sd).reshape(-1)
    gm = np.zeros((T, Dr)); gs = np.zeros((T, Dr))
    for k, c in enumerate(cols):
        hh = 2 * h * max(1.0, abs(Xr[:, c]).max())
        p, m = slice((1 + 2 * k) * T, (2 + 2 * k) * T), slice((2 + 2 * k) * T, (3 + 2 * k) * T)
        gm[:, c] = (mu[p] - mu[m]) / hh; gs[:, c] = (sd[p] - sd[m]) / hh
    return gm, gs


@pytest.mark.parametrize('xalgo', Scaler.algos)
def test_raw_mode_through_every_x_scaler(xalgo):
    eng, xs, ys, alpha, Li, Xr = _scaled_problem(xalgo, 'normal')
    mu, sd, dmu, dsd = eng.predict_grad(Xr, alpha, Li, mode='raw')
    mu_r, sd_r = eng.predict_raw(Xr, alpha, Li)
    assert np.array_equal(mu, mu_r) and np.array_equal(sd, sd_r)
    assert dmu.shape == (Xr.shape[0], 4) and np.all(dmu[:, 2] == 0) and np.all(dsd[:, 2] == 0)
    # the chain: the scaled gradients times the Jacobian of the forward transform
    _, _, gmu, gsd = eng.predict_grad(np.ascontiguousarray(xs.forward_transform(Xr)), alpha, Li)
    Jx = R.x_scaler_deriv(xs, Xr)
    cols = xs.data['cols']
    assert rel(dmu[:, cols], gmu * Jx) < 1e-12 and rel(dsd[:, cols], gsd * Jx) < 1e-12
    fm, fs = _fd(lambda X: eng.predict_raw(X, alpha, Li), Xr, cols)
    assert rel(dmu, fm) < 1e-5 and rel(dsd, fs) < 1e-5
    eng.close()


@pytest.mark.parametrize('yalgo', Scaler.algos)
def test_y_mode_through_every_y_scaler(yalgo):
    eng, xs, ys, alpha, Li, Xr = _scaled_problem('auto-inv-normal' if yalgo != 'min-max' else 'normal', yalgo)
    mu, sd, dmu, dsd = eng.predict_grad(Xr, alpha, Li, mode='y')
    mu_y, sd_y, _ = eng.predict_y(Xr, alpha, Li)
    assert np.array_equal(mu, mu_y, equal_nan=True) and np.array_equal(sd, sd_y.ravel(), equal_nan=True)
    fm, fs = _fd(lambda X: eng.predict_y(X, alpha, Li)[:2], Xr, xs.data['cols'])
    # inv-normal y scalers map through the normal ppf: a band mu +- std that leaves (0, 1) has no finite std_y (nor gradient)
    ok = np.isfinite(sd) & np.isfinite(fs).all(1)
    assert ok.sum() >= len(ok) // 2 and np.isfinite(dsd[ok]).all()
    assert rel(dmu[ok], fm[ok]) < 1e-5 and rel(dsd[ok], fs[ok]) < 1e-5
    _, _, dmu1, _ = eng.predict_grad(Xr, alpha, Li, mode='y', want_std=False)
    assert np.array_equal(dmu1, dmu, equal_nan=True)
    eng.close()


def test_f16x3_context_equals_fp32_context():
    D, S, M, T = 64, 32, 1024, 40000
    e32, params, alpha, Li = _engine(D, S, M, 'f32')
    from scfgp_amd.engine import HipEngine
    e16 = HipEngine(D, S, M, dtype='f16x3'); e16.set_params(params)
    Xs = synth.make_X(202, T, D)
    a = e32.predict_grad(Xs, alpha, Li)
    b = e16.predict_grad(Xs, alpha, Li)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    e32.close(); e16.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_training_state_survives(dtype):
    eng, params, alpha, Li = _engine(20, 20, 280, dtype)
    c0, g0, a0, L0 = eng.eval(want_grad=True)
    c0, g0, a0, L0 = float(c0), g0.copy(), a0.copy(), L0.copy()
    eng.predict_grad(synth.make_X(9, 33000, 20), alpha, Li)
    c1, g1, a1, L1 = eng.eval(want_grad=True)
    assert float(c1) == c0 and np.array_equal(g1, g0) and np.array_equal(a1, a0) and np.array_equal(L1, L0)
    eng.close()


def test_errors():
    eng, params, alpha, Li = _engine(5, 4, 60, 'f64', N=300)
    Xs = synth.make_X(3, 10, 5)
    with pytest.raises(ValueError):
        eng.predict_grad(Xs, alpha, Li, mode='raw')                     # no X scaler registered
    with pytest.raises(ValueError):
        eng.predict_grad(Xs, alpha, Li, mode='bogus')
    eng.close()


def test_facade_predict_grad():
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
    mu, sd, dmu, dsd = model.predict_grad(Xs)
    assert mu.shape == (60, 1) and sd.shape == (60, 1) and dmu.shape == (60, 4) and dsd.shape == (60, 4)
    mu_p, sd_p = model.predict(Xs)
    assert np.array_equal(mu, mu_p) and np.array_equal(sd, sd_p)
    assert np.all(dmu[:, 2] == 0) and np.all(dsd[:, 2] == 0)
    fm, fs = _fd(model.predict, Xs, [0, 1, 3])
    assert rel(dmu, fm) < 1e-5 and rel(dsd, fs) < 1e-5
    other = SCFGP(sparsity=3, nfeats=12)
    other.pred_func = lambda Xs, alpha, Li: None
    with pytest.raises(TypeError):
        other.predict_grad(Xs)
