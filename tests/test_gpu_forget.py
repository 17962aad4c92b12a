"""GPU tier of the posterior downdate (scfgp_forget): parity of the device downdate, fed the oracle's fit of ALL rows, with the oracle's
fit on the remaining rows under the project's per-tile bounds (tests/parity.py: TOL, unchanged); device fit -> condition -> forget
against the device fit; the bit-level guarantees (zeros above the diagonal, aliasing, f16x3 = fp32, mu / std = predict with the
returned factors, the predictions-only form); agreement with scfgp_loo on consecutive blocks; the errors and the survival of the
training state; and the SCFGP.forget / SCFGP.cv facade."""
import functools

import numpy as np
import pytest

from oracle import scfgp_oracle as O
from scfgp_amd import synth
from scfgp_amd.scaler import Scaler
from tests import condition_ref as CR
from tests import forget_ref as R
from tests import loo_ref
from tests import parity

pytestmark = pytest.mark.gpu

# (D, S, M, N0, n): n rows leave a fit on N0 + n.  tests/test_forget_ref.py's first five, K = 2112, and one whose removed rows fill two
# chunks of 32 768 and leave a ragged third (a half of the upload buffer is reused, in both passes)
SHAPES = [(5, 4, 60, 1000, 300), (5, 4, 60, 1000, 1), (20, 20, 280, 3000, 700), (3, 1, 20, 150, 400), (40, 4, 100, 2000, 129),
          (64, 32, 1024, 4000, 900), (5, 4, 60, 1000, 65536 + 300)]
THREE_CHUNKS = SHAPES[6]


@functools.lru_cache(maxsize=None)
def _fits(D, S, M, N0, n):
    params, X, y, Xs = CR.problem(D, S, M, N0, n)
    _, a0, L0 = O.forward(X[:N0], y[:N0], params, S, M, gauss_hermite=False)
    _, a1, L1 = O.forward(X, y, params, S, M, gauss_hermite=False)
    mu0, sd0 = O.predict(Xs, a0, L0, params, S, M)
    return params, X, y, Xs, a0, L0, a1, L1, mu0, sd0


def _engine(D, S, M, dtype, params):
    from scfgp_amd.engine import HipEngine
    eng = HipEngine(D, S, M, dtype=dtype); eng.set_params(params)
    return eng


def _checks(eng, al, Li, a0, L0, Xs, mu0, sd0, tol, label):
    mu, sd = eng.predict(Xs, al, Li)
    r = dict(alpha=parity.alpha_ratio(al, a0, tol), Li=parity.li_ratio(Li, L0, tol), predict=parity.predict_ratio(mu, sd, mu0, sd0, tol))
    print(label, tol, parity.fmt(r))
    parity.check_alpha(al, a0, tol); parity.check_li(Li, L0, tol); parity.check_predict(mu, sd, mu0, sd0, tol)
    return r


def _same_stats(s, t):
    return all(np.array_equal(s[k], t[k]) for k in s) and s.keys() == t.keys()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('D,S,M,N0,n', SHAPES)
def test_parity_with_the_oracle_fit_on_the_remaining_rows(D, S, M, N0, n, dtype):
    """the device downdate is fed the ORACLE's factors of all N0 + n rows, so only the downdate's own error is measured"""
    params, X, y, Xs, a0, L0, a1, L1, mu0, sd0 = _fits(D, S, M, N0, n)
    eng = _engine(D, S, M, dtype, params)
    al, Li, mu, sd, st = eng.forget(X[N0:], y[N0:], a1, L1, factors=True, predict=True)
    assert al.shape == (2 * (S + M), 1) and Li.shape == L0.shape and mu.shape == (n, 1) and sd.shape == (n,)
    assert np.all(np.triu(Li, 1) == 0.0)                                 # exactly zero above the diagonal
    print('min M_ii^2 %.3f' % st['min_pivot2'])
    assert st['n'] == n and st['blocks'] == 1 and 0.0 < st['min_pivot2'] <= 1.0
    _checks(eng, al, Li, a0, L0, Xs, mu0, sd0, dtype, 'forget %s' % ((D, S, M, N0, n),))
    assert parity.alpha_ratio(a1, a0, 'f32') > 1.0                       # the un-downdated factors fail even the looser bound
    # mu, std: bit for bit predict with the returned factors (here also at the three-chunk shape)
    mu2, sd2 = eng.predict(X[N0:], al, Li)
    assert np.array_equal(mu, mu2) and np.array_equal(sd, sd2)
    eng.close()


# The round trip's third shape sends three chunks through both calls and keeps as many rows as it removes.  The downdate divides the
# error of the factors it is GIVEN by lam_min(S) ~ N0 / (N0 + n), and here they are scfgp_condition's: in an fp32 context its fp32 Gram
# leaves about a tenth of the predict bound in them (tests/test_gpu_condition.py prints it).  With N0 = 1000 kept of 66 836 that is
# multiplied by 67 and the round trip cannot hold the fp32 bound whatever scfgp_forget does (measured: predict ratio 1.4, fp64 context
# 2e-4); with N0 = 66 000 it is multiplied by 2.
ROUND_TRIP = [SHAPES[0], SHAPES[2], (5, 4, 60, 66000, 65536 + 300)]


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('D,S,M,N0,n', ROUND_TRIP)
def test_device_fit_condition_forget_returns_to_the_device_fit(D, S, M, N0, n, dtype):
    params, X, y, Xs = CR.problem(D, S, M, N0, n)
    eng = _engine(D, S, M, dtype, params)
    _, _, a0, L0 = eng.eval(np.ascontiguousarray(X[:N0]), np.ascontiguousarray(y[:N0]), want_grad=False)
    a0, L0 = a0.copy(), L0.copy()
    mu0, sd0 = eng.predict(Xs, a0, L0)
    ac, Lc = eng.condition(X[N0:], y[N0:], a0, L0)
    al, Li = eng.forget(X[N0:], y[N0:], ac, Lc)
    _checks(eng, al, Li, a0, L0, Xs, mu0, sd0, dtype, 'round trip %s' % ((D, S, M, N0, n),))
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_aliasing_upper_entries_and_the_predictions_only_form(dtype):
    from scfgp_amd._lib import dptr
    D, S, M, N0, n = SHAPES[2]
    params, X, y, Xs, a0, L0, a1, L1, *_ = _fits(D, S, M, N0, n)
    eng = _engine(D, S, M, dtype, params)
    al, Li, mu, sd, st = eng.forget(X[N0:], y[N0:], a1, L1, factors=True, predict=True)
    # entries above the diagonal of the incoming factor are not read
    al2, Li2 = eng.forget(X[N0:], y[N0:], a1, L1 + np.triu(np.full_like(L1, 7.0), 1))
    assert np.array_equal(al2, al) and np.array_equal(Li2, Li)
    # the predictions-only call returns the same mu / std / stats bits as the full call
    mu3, sd3, st3 = eng.forget(X[N0:], y[N0:], a1, L1, factors=False, predict=True)
    assert np.array_equal(mu3, mu) and np.array_equal(sd3, sd) and _same_stats(st3, st)
    # the stats' sums are those of the rounded outputs in row order
    e = y[N0:].ravel() - mu.ravel()
    assert st['sum_e2'] == functools.reduce(lambda s, v: s + v, (e * e).tolist(), 0.0)
    assert st['sum_abs_e'] == functools.reduce(lambda s, v: s + v, np.abs(e).tolist(), 0.0)
    marg = -0.5 * (e * e / (sd * sd) + np.log(2 * np.pi * (sd * sd)))
    assert abs(st['sum_log_marginal'] - np.sum(marg)) <= 1e-12 * np.sum(np.abs(marg))
    # aliased factor outputs
    Xo = np.ascontiguousarray(X[N0:]); yo = np.ascontiguousarray(y[N0:]).ravel()
    a = np.ascontiguousarray(a1).ravel().copy(); L = np.ascontiguousarray(L1).copy()
    eng._check(eng.lib.scfgp_forget(eng.ctx, dptr(Xo), dptr(yo), n, dptr(a), dptr(L), 0, dptr(a), dptr(L), None, None, None), 'forget')
    assert np.array_equal(a, al.ravel()) and np.array_equal(L, Li)
    eng.close()


def test_f16x3_equals_fp32_bit_for_bit():
    D, S, M, N0, n = SHAPES[5]
    params, X, y, Xs, a0, L0, a1, L1, *_ = _fits(D, S, M, N0, n)
    out = []
    for dtype in ('f32', 'f16x3'):
        eng = _engine(D, S, M, dtype, params)
        out.append(eng.forget(X[N0:], y[N0:], a1, L1, factors=True, predict=True))
        eng.close()
    for u, v in zip(out[0][:4], out[1][:4]):
        assert np.array_equal(u, v)
    assert _same_stats(out[0][4], out[1][4])


def _scaled_problem(xalgo, yalgo, dtype='f64', seed=5, N=600):
    """tests/test_gpu_condition.py's problem: an engine fitted on scaled data of 4 raw columns, one of them constant"""
    from scfgp_amd.engine import HipEngine
    rng = np.random.default_rng(seed)
    Xr = np.column_stack([rng.uniform(0.5, 3.0, N), rng.gamma(2.0, 1.0, N), np.full(N, 2.5), rng.normal(1.0, 2.0, N)])
    yr = np.exp(0.3 * np.sin(Xr[:, :1]) + 0.1 * Xr[:, 1:2]) + 0.05 * rng.standard_normal((N, 1))
    xs = Scaler(xalgo); xs.fit(Xr); ys = Scaler(yalgo); ys.fit(yr)
    D, S, M = 3, 2, 40
    eng = HipEngine(D, S, M, dtype=dtype)
    eng.set_params(synth.make_params(seed, D, S, M, abc=(-1.0, 0.0, -4.0)))
    eng.set_data(np.ascontiguousarray(xs.forward_transform(Xr)), np.ascontiguousarray(ys.forward_transform(yr)))
    _, _, alpha, Li = eng.eval(want_grad=False)
    eng.set_x_scaler(xs); eng.set_y_scaler(ys)
    return eng, xs, ys, alpha.copy(), Li.copy(), Xr, yr


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_raw_mode_predictions_are_predict_raw_bit_for_bit(dtype):
    eng, xs, ys, alpha, Li, Xr, yr = _scaled_problem('normal', 'normal', dtype)
    fy = np.asarray(ys.forward_transform(yr))
    rows = np.arange(40, 160)
    al, Ln, mu, sd, st = eng.forget(Xr[rows], fy[rows], alpha, Li, factors=True, predict=True, mode='raw')
    mu2, sd2 = eng.predict_raw(Xr[rows], al, Ln)
    assert np.array_equal(mu, mu2) and np.array_equal(sd, sd2)
    rel = lambda a, b: float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))
    assert rel(al, alpha) > 1e-6                                                    # the rows did move the posterior
    if dtype == 'f64':
        # ... and close to scaled mode on the host-transformed rows: both are fp64 evaluations of the same element-wise formula, the
        # 1e-12 of tests/test_gpu_condition.py's test of the two modes (in fp32 a last-bit difference of a row flips fp32 roundings)
        a0, L0 = eng.forget(np.ascontiguousarray(xs.forward_transform(Xr[rows])), fy[rows], alpha, Li)
        assert rel(al, a0) < 1e-12 and rel(Ln, L0) < 1e-12
    eng.close()


def _rel(a, b):
    a = np.asarray(a, np.float64).ravel(); b = np.asarray(b, np.float64).ravel()
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


LOO_BLOCKS = (1, 7, 64)


@functools.lru_cache(maxsize=None)
def _loo_reference_deviation():
    """The fp32 tolerance's source: the worst deviation, over mu, std and the joint density of the three blocks, of forget_ref run with
    the C an fp32 context holds from loo_ref at this shape, computed on the CPU.  That C is tests/parity.apply32_model's: fp32 Phi times
    fp32 Li^T, accumulated and stored in fp32 -- what scfgp_loo's C is in an fp32 context, while scfgp_forget's first pass is fp64
    there.  Per block 1 / 7 / 64 it is 7.1e-10 / 6.1e-9 / 1.2e-8.  (Rounding the exact C to fp32 ONCE instead leaves out the
    accumulation over K = 600 terms and gives 2.0e-10 / 4.7e-10 / 1.6e-9; the device's 3.6e-9 / 8.7e-9 for block 1 / 7 exceed four
    times those, and neither model holds the fp32 predict pass that forms scfgp_forget's mu and std.)"""
    D, S, M, N0, n = SHAPES[2]
    params, X, y, Xs, a0, L0, a1, L1, *_ = _fits(D, S, M, N0, n)
    i0 = 448
    worst = 0.0
    for block in LOO_BLOCKS:
        ref = loo_ref.loo(X[i0:i0 + block], y[i0:i0 + block], a1, L1, params, S, M, block=block)
        out = R.forget(X[i0:i0 + block], y[i0:i0 + block], a1, L1, params, S, M, C_model=parity.apply32_model)
        d = max(_rel(out['mu'], ref['mu']), _rel(out['std'], ref['std']), _rel(out['stats'][4], ref['joint'][0]))
        print('forget_ref with an fp32 C against loo_ref, block %d: %.3g' % (block, d))
        worst = max(worst, d)
    return worst


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('block', LOO_BLOCKS)
def test_agrees_with_scfgp_loo_on_a_block_of_consecutive_rows(block, dtype):
    """fp64 contexts: 1e-8 (max-norm relative).  fp32 contexts: 4 x the worst deviation of forget_ref with an fp32 context's C from
    loo_ref at this shape, computed on the CPU (_loo_reference_deviation: one number for the shape)."""
    D, S, M, N0, n = SHAPES[2]
    params, X, y, Xs, a0, L0, a1, L1, *_ = _fits(D, S, M, N0, n)
    i0 = 448
    Xb, yb = X[i0:i0 + block], y[i0:i0 + block]
    eng = _engine(D, S, M, dtype, params)
    mu, sd, st = eng.forget(Xb, yb, a1, L1, factors=False, predict=True)
    mu_l, sd_l, _, st_l = eng.loo(Xb, yb, a1, L1, block=block)
    d = dict(mu=_rel(mu, mu_l), std=_rel(sd, sd_l), joint=_rel(st['log_joint'], st_l['sum_log_joint']))
    tol = 1e-8 if dtype == 'f64' else 4.0 * _loo_reference_deviation()
    print('loo block %d %s' % (block, dtype), d, 'tolerance %.3g' % tol)
    assert max(d.values()) <= tol
    eng.close()


def test_errors_leave_the_outputs_untouched():
    from scfgp_amd.engine import HipEngine
    from scfgp_amd._lib import dptr
    D, S, M, N0, n = SHAPES[0]
    params, X, y, Xs, a0, L0, a1, L1, mu0, sd0 = _fits(D, S, M, N0, n)
    eng = _engine(D, S, M, 'f64', params)
    Xo = np.ascontiguousarray(X[N0:]); yo = np.ascontiguousarray(y[N0:]).ravel()
    a = np.ascontiguousarray(a1).ravel()
    Xt, yt, k, h = R.tiled_row(X, y, a1, L1, params, S, M, i=3)
    Xt = np.ascontiguousarray(Xt); yt = np.ascontiguousarray(yt)
    rows = max(n, k)
    outs = [np.full(a.size, 3.0), np.full(L1.shape, 3.0), np.full(rows, 3.0), np.full(rows, 3.0), np.full(8, 3.0)]

    def lib_call(X_, y_, n_, a_, L_, mode, drop=()):
        o = [None if i in drop else dptr(v) for i, v in enumerate(outs)]
        eng._check(eng.lib.scfgp_forget(eng.ctx, dptr(X_), dptr(y_), n_, dptr(a_), dptr(L_), mode, *o), 'forget')
    for bad in (np.nan, np.inf):
        yb = yo.copy(); yb[17] = bad
        with pytest.raises(FloatingPointError, match='non-finite'):
            lib_call(Xo, yb, n, a, L1, 0)
        with pytest.raises(FloatingPointError, match='non-finite'):
            eng.forget(Xo, yb, a1, L1)
    Xb = Xo.copy(); Xb[3, 2] = np.nan
    with pytest.raises(FloatingPointError, match='non-finite'):
        lib_call(Xb, yo, n, a, L1, 0)
    Lb = L1.copy(); Lb[50, 3] = np.inf
    with pytest.raises(FloatingPointError, match='non-finite'):
        lib_call(Xo, yo, n, a, Lb, 0)
    ab = a.copy(); ab[5] = np.nan
    with pytest.raises(FloatingPointError, match='non-finite'):
        lib_call(Xo, yo, n, ab, L1, 0)
    # one fit row tiled k times, k h >= 2: S = I - k c c^T has no Cholesky factor
    assert k * h >= 2.0
    with pytest.raises(np.linalg.LinAlgError, match='not in this fit'):
        lib_call(Xt, yt, k, a, L1, 0)
    assert eng.lib.scfgp_forget(eng.ctx, dptr(Xt), dptr(yt), k, dptr(a), dptr(L1), 0, *[dptr(v) for v in outs]) == -3
    with pytest.raises(ValueError, match='n must be at least 1'):
        lib_call(Xo, yo, 0, a, L1, 0)
    with pytest.raises(ValueError, match='bad arguments'):
        lib_call(Xo, yo, n, a, L1, 2)
    with pytest.raises(ValueError, match='bad arguments'):
        lib_call(Xo, None, n, a, L1, 0)
    with pytest.raises(ValueError, match='alpha_out and Li_out go together'):
        lib_call(Xo, yo, n, a, L1, 0, drop=(1,))
    with pytest.raises(ValueError, match='mu and std go together'):
        lib_call(Xo, yo, n, a, L1, 0, drop=(2,))
    with pytest.raises(ValueError, match='stats need mu and std'):
        lib_call(Xo, yo, n, a, L1, 0, drop=(2, 3))
    with pytest.raises(ValueError, match='no output asked for'):
        lib_call(Xo, yo, n, a, L1, 0, drop=(0, 1, 2, 3, 4))
    with pytest.raises(ValueError, match='no X scaler'):
        lib_call(Xo, yo, n, a, L1, 1)
    assert all(np.all(o == 3.0) for o in outs)                           # the outputs are untouched by every failure
    with pytest.raises(ValueError, match='columns'):
        eng.forget(Xo[:, :4], yo, a1, L1)
    with pytest.raises(ValueError, match='entries'):
        eng.forget(Xo, yo[:-1], a1, L1)
    with pytest.raises(ValueError, match='shape'):
        eng.forget(Xo, yo, a1, L1[:-1])
    with pytest.raises(ValueError, match='scaler'):
        eng.forget(Xo, yo, a1, L1, mode='raw')
    with pytest.raises(ValueError):
        eng.forget(Xo, yo, a1, L1, factors=False, predict=False)
    al, Li = eng.forget(Xo, yo, a1, L1)                                  # the context still works
    _checks(eng, al, Li, a0, L0, Xs, mu0, sd0, 'f64', 'after the errors')
    eng.close()
    fresh = HipEngine(D, S, M, dtype='f64')                              # no parameters yet
    with pytest.raises(ValueError, match='parameters not set'):
        fresh.forget(Xo, yo, a1, L1)
    fresh.close()


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
    eng.forget(X[:300], y[:300], a0, L0, factors=True, predict=True)
    eng.forget(X[300:307], y[300:307], a0, L0, factors=False, predict=True)
    c1, g1, a1, L1 = eng.eval(want_grad=True)
    assert float(c1) == c0 and np.array_equal(g1, g0) and np.array_equal(a1, a0) and np.array_equal(L1, L0)
    eng.close()
    # two successive scfgp_train calls, with and without a downdate between them
    runs = []
    for between in (False, True):
        eng = HipEngine(D, S, M, dtype=dtype); eng.set_params(params); eng.set_data(X, y)
        eng.opt_init('adam', learning_rate=0.01)
        h1, al, Li = eng.train(3)
        if between:
            # (al, Li) are those of the iteration before the last step, so for the parameters the context holds now these rows are
            # only nearly rows of the fit: three of them (leverage about K / N = 0.4 each) leave S far from singular all the same
            eng.forget(X[:3], y[:3], al, Li, factors=True, predict=True)
        h2, al2, Li2 = eng.train(3)
        runs.append((h1.copy(), h2.copy(), eng.get_params().copy(), al2.copy(), Li2.copy()))
        eng.close()
    for u, v in zip(*runs):
        assert np.array_equal(u, v)


def _fitted_model(N=400):
    from scfgp_amd import SCFGP
    rng = np.random.default_rng(5)
    np.random.seed(5)
    X = rng.uniform(-2, 2, (N, 3))
    X = np.column_stack([X[:, :2], np.full(N, 4.0), X[:, 2:]])          # a constant column
    y = np.sin(X[:, :1]) + 0.5 * X[:, 1:2] ** 2 + 0.05 * rng.standard_normal((N, 1))
    model = SCFGP(sparsity=3, nfeats=12, device_scaler=True)
    model.fit(X, y, max_iter=20,
              algo={'algo': 'adam', 'algo_params': {'learning_rate': 0.02, 'beta1': 0.9, 'beta2': 0.999, 'epsilon': 1e-8}})
    return model, X, y


def _y_units(model, mu_f, sd_f):
    mu_f = np.asarray(mu_f).reshape(-1, 1); sd_f = np.asarray(sd_f).reshape(-1, 1)
    b = model.y_scaler.backward_transform
    return b(mu_f), 0.5 * (b(mu_f + sd_f) - b(mu_f - sd_f))


def test_facade_cv_equals_explicit_refits():
    """SCFGP.cv(folds=4) against four refits on the other three folds at the model's parameters and scalers (train_func on the
    remaining scaled rows, pred_func on the fold), in raw y units"""
    model, X, y = _fitted_model()
    a_before, L_before = np.array(model.alpha), np.array(model.Li)
    mu_y, std_y, metrics, fold_stats = model.cv(folds=4, seed=3)
    assert mu_y.shape == (400, 1) and std_y.shape == (400, 1) and len(fold_stats) == 4
    assert sum(st['n'] for st in fold_stats) == 400 and sorted(st['n'] for st in fold_stats) == [100] * 4
    assert np.array_equal(model.alpha, a_before) and np.array_equal(model.Li, L_before)
    ids = np.empty(400, dtype=np.int64)
    ids[np.random.default_rng(3).permutation(400)] = np.arange(400) % 4
    fx = np.asarray(model.X); fy = np.asarray(model.y)
    mu_r = np.empty((400, 1)); sd_r = np.empty((400, 1))
    for f in range(4):
        keep, rows = np.flatnonzero(ids != f), np.flatnonzero(ids == f)
        _, a, L = model.train_func(np.ascontiguousarray(fx[keep]), np.ascontiguousarray(fy[keep]))
        m, s = model.pred_func(np.ascontiguousarray(fx[rows]), a, L)
        mu_r[rows], sd_r[rows] = _y_units(model, m, s)
    print('cv predict ratio', parity.predict_ratio(mu_y, std_y, mu_r, sd_r, 'f64'), {k: float(v) for k, v in metrics.items()})
    parity.check_predict(mu_y, std_y, mu_r, sd_r, 'f64')
    # the same folds given as ids, and the raw rows passed explicitly: the same predictions
    mu2, sd2, _, _ = model.cv(folds=ids)
    assert np.array_equal(mu2, mu_y) and np.array_equal(sd2, std_y)
    mu3, sd3, _, _ = model.cv(X, y, folds=ids)
    parity.check_predict(mu3, sd3, mu_r, sd_r, 'f64')
    with pytest.raises(ValueError):
        model.cv(folds=1)
    with pytest.raises(ValueError):
        model.cv(folds=ids[:-1])


def test_facade_forget_after_condition_restores_predict():
    model, X, y = _fitted_model()
    rng = np.random.default_rng(11)
    Xn = rng.uniform(-2, 2, (90, 3)); Xn = np.column_stack([Xn[:, :2], np.full(90, 4.0), Xn[:, 2:]])
    yn = np.sin(Xn[:, :1]) + 0.5 * Xn[:, 1:2] ** 2
    Xs = X[:60] + 0.01
    fs = np.ascontiguousarray(model.X_scaler.forward_transform(Xs), dtype=np.float64)
    mu0, sd0 = model.pred_func(fs, model.alpha, model.Li)
    a0 = np.array(model.alpha)
    model.condition(Xn, yn)
    assert not np.array_equal(model.alpha, a0)
    assert model.forget(Xn, yn) is model
    mu, sd = model.pred_func(fs, model.alpha, model.Li)
    print('facade round trip predict ratio', parity.predict_ratio(mu, sd, mu0, sd0, 'f64'))
    parity.check_predict(mu, sd, mu0, sd0, 'f64')
    from scfgp_amd import SCFGP
    other = SCFGP(sparsity=3, nfeats=12)
    other.pred_func = lambda Xs, alpha, Li: None
    with pytest.raises(TypeError):
        other.forget(X[:5], y[:5])
    with pytest.raises(TypeError):
        other.cv(folds=2)
