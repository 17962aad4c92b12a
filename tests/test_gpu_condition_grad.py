"""GPU tier of scfgp_condition_grad: parity of the device update, fed the oracle's fit of N0 rows, with the fp64 closed form on the
oracle's feature map (tests/condition_grad_ref.py) under the project's per-tile bounds (tests/parity.py: check_alpha, check_li,
check_predict, unchanged: the call runs scfgp_condition's products); three-chunk calls; rho = 0; composition with scfgp_condition and
scfgp_predict_grad; the bit-level and state guarantees; raw mode; the SCFGP.condition_grad facade; and the errors.

The derivative rows carry the norm of F_all's rows and of sqrt(rho): |psi_d| = |F_all[d, :]| sqrt(rho / J) |phi|.  With the update's
first pass in the context's fp32 products the fp64 runs of these cases stayed at rounding level while fp32 runs left the fp32 bound of
check_predict: ratio 6.9 at (64, 32, 1024) with rho = NULL and 200 with the drawn rho (100 among its values), 1.3 .. 1.6 at (7, 12, 3) and
(16, 16, 70) with the drawn rho.  The bounds stand; the library runs the first pass in fp64 in every context instead, as scfgp_forget
does, and the fp32 cases below hold that path to the fp32 bounds."""
import functools

import numpy as np
import pytest

from oracle import scfgp_oracle as O
from scfgp_amd import synth
from scfgp_amd.scaler import Scaler
from tests import condition_grad_ref as R
from tests import parity
from tests.test_gpu_predict_grad import BOUNDS as DMU_BOUNDS

pytestmark = pytest.mark.gpu

def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


@functools.lru_cache(maxsize=None)
def _case(D, S, M, N0, n, dims):
    p = R.problem(D, S, M, N0, n, dims)
    _, a0, L0 = O.forward(p['X0'], p['y0'], p['params'], S, M, gauss_hermite=False)
    return p, a0, L0


@functools.lru_cache(maxsize=None)
def _reference(shape, with_y, rho_kind):
    """(alpha', Li', mu, sd on the held-out rows) of the closed form; rho_kind: None or 'drawn'"""
    D, S, M, N0, n, dims = shape
    p, a0, L0 = _case(*shape)
    a1, L1 = R.condition_grad(p['Xn'], p['G'], a0, L0, p['params'], S, M, dims=dims, rho=_rho(shape, rho_kind), y=p['yn'] if with_y else None)
    mu1, sd1 = O.predict(p['Xs'], a1, L1, p['params'], S, M)
    return a1, L1, mu1, sd1


def _rho(shape, kind):
    D, S, M, N0, n, dims = shape
    p, _, _ = _case(*shape)
    return None if kind is None else p['rho']


def _engine(D, S, M, dtype, params):
    from scfgp_amd.engine import HipEngine
    eng = HipEngine(D, S, M, dtype=dtype); eng.set_params(params)
    return eng


def _checks(eng, al, Li, ref, Xs, tol, label):
    a1, L1, mu1, sd1 = ref
    mu, sd = eng.predict(Xs, al, Li)
    r = dict(alpha=parity.alpha_ratio(al, a1, tol), Li=parity.li_ratio(Li, L1, tol), predict=parity.predict_ratio(mu, sd, mu1, sd1, tol))
    print(label, tol, parity.fmt(r))
    parity.check_alpha(al, a1, tol); parity.check_li(Li, L1, tol); parity.check_predict(mu, sd, mu1, sd1, tol)
    return r


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('with_rho', [False, True], ids=['ones', 'rho'])
@pytest.mark.parametrize('with_y', [False, True], ids=['grad', 'grad+y'])
@pytest.mark.parametrize('i', range(len(R.SHAPES)))
def test_parity_with_the_closed_form(i, with_y, with_rho, dtype):
    """the device update is fed the ORACLE's factors of the N0 rows, so only the update's own error is measured"""
    shape = R.SHAPES[i]
    D, S, M, N0, n, dims = shape
    p, a0, L0 = _case(*shape)
    kind = 'drawn' if with_rho else None
    eng = _engine(D, S, M, dtype, p['params'])
    al, Li = eng.condition_grad(p['Xn'], p['G'], a0, L0, dims=dims, rho=_rho(shape, kind), y=p['yn'] if with_y else None)
    assert al.shape == (2 * (S + M), 1) and Li.shape == L0.shape
    assert np.all(np.triu(Li, 1) == 0.0)                                 # exactly zero above the diagonal
    _checks(eng, al, Li, _reference(shape, with_y, kind), p['Xs'], dtype, 'condition_grad %s y=%d rho=%s' % (shape, with_y, kind))
    eng.close()


# nb = 6 -> 5461 points per chunk; nb = 71 -> 461: two full chunks and a ragged one of 3 points (a half of the feed is reused)
CHUNKED = [(5, 4, 60, 1000, 2 * 5461 + 3, None), (70, 5, 60, 2000, 2 * 461 + 3, None)]


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('shape', CHUNKED, ids=['nb6', 'nb71'])
def test_three_chunk_calls(shape, dtype):
    D, S, M, N0, n, dims = shape
    p, a0, L0 = _case(*shape)
    eng = _engine(D, S, M, dtype, p['params'])
    assert n == 2 * eng.condition_grad_points_per_chunk(D, True) + 3
    al, Li = eng.condition_grad(p['Xn'], p['G'], a0, L0, rho=p['rho'], y=p['yn'])
    _checks(eng, al, Li, _reference(shape, True, 'drawn'), p['Xs'], dtype, 'three chunks %s' % (shape,))
    al2, Li2 = eng.condition_grad(p['Xn'], p['G'], a0, L0, rho=p['rho'], y=p['yn'])
    assert np.array_equal(al2, al) and np.array_equal(Li2, Li)          # the same bits from run to run
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_rho_zero_contributes_nothing_and_ones_equal_null(dtype):
    shape = R.SHAPES[1]
    D, S, M, N0, n, dims = shape
    p, a0, L0 = _case(*shape)
    eng = _engine(D, S, M, dtype, p['params'])
    zero = p['rho'] == 0
    assert zero.any()
    out = eng.condition_grad(p['Xn'], p['G'], a0, L0, rho=p['rho'], y=p['yn'])
    for fill in (-3.0e5, 1e-300, 7.0):
        G2 = p['G'].copy(); G2[zero] = fill
        other = eng.condition_grad(p['Xn'], G2, a0, L0, rho=p['rho'], y=p['yn'])
        assert np.array_equal(other[0], out[0]) and np.array_equal(other[1], out[1])
    for y in (None, p['yn']):
        a = eng.condition_grad(p['Xn'], p['G'], a0, L0, y=y)
        b = eng.condition_grad(p['Xn'], p['G'], a0, L0, rho=np.ones_like(p['G']), y=y)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_composition_with_condition_and_predict_grad(dtype):
    shape = R.SHAPES[1]
    D, S, M, N0, n, dims = shape
    p, a0, L0 = _case(*shape)
    ref = _reference(shape, True, 'drawn')
    eng = _engine(D, S, M, dtype, p['params'])
    av, Lv = eng.condition(p['Xn'], p['yn'], a0, L0)
    two = eng.condition_grad(p['Xn'], p['G'], av, Lv, rho=p['rho'])
    one = eng.condition_grad(p['Xn'], p['G'], a0, L0, rho=p['rho'], y=p['yn'])
    _checks(eng, two[0], two[1], ref, p['Xs'], dtype, 'values, then derivatives')
    _checks(eng, one[0], one[1], ref, p['Xs'], dtype, 'one call')
    dmu = eng.predict_grad(p['Xn'], one[0], one[1], want_std=False)[2]
    e = rel(dmu, R.mean_grad(p['Xn'], ref[0], p['params'], S, M))
    print('updated mean gradient', dtype, e)
    assert e < DMU_BOUNDS[dtype][0]
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_outputs_may_alias_the_inputs(dtype):
    from scfgp_amd._lib import dptr
    import ctypes as C
    shape = R.SHAPES[3]                                                  # dims (6, 0, 3): the explicit list goes through the library
    D, S, M, N0, n, dims = shape
    p, a0, L0 = _case(*shape)
    eng = _engine(D, S, M, dtype, p['params'])
    al, Li = eng.condition_grad(p['Xn'], p['G'], a0, L0, dims=dims, rho=p['rho'], y=p['yn'])
    # entries above the diagonal of the incoming factor are not read
    al2, Li2 = eng.condition_grad(p['Xn'], p['G'], a0, L0 + np.triu(np.full_like(L0, 7.0), 1), dims=dims, rho=p['rho'], y=p['yn'])
    assert np.array_equal(al2, al) and np.array_equal(Li2, Li)
    a = np.ascontiguousarray(a0).ravel().copy(); L = np.ascontiguousarray(L0).copy()
    d32 = np.array(dims, dtype=np.int32)
    G = np.ascontiguousarray(p['G']); rho = np.ascontiguousarray(p['rho']); X = np.ascontiguousarray(p['Xn']); y = np.ascontiguousarray(p['yn'])
    eng._check(eng.lib.scfgp_condition_grad(eng.ctx, dptr(X), n, d32.ctypes.data_as(C.POINTER(C.c_int32)), len(dims), dptr(G), dptr(rho),
                                            dptr(y), dptr(a), dptr(L), 0, dptr(a), dptr(L)), 'condition_grad')
    assert np.array_equal(a, al.ravel()) and np.array_equal(L, Li)
    eng.close()


def test_f16x3_equals_fp32_bit_for_bit():
    shape = R.SHAPES[6]
    D, S, M, N0, n, dims = shape
    p, a0, L0 = _case(*shape)
    out = []
    for dtype in ('f32', 'f16x3'):
        eng = _engine(D, S, M, dtype, p['params'])
        out.append(eng.condition_grad(p['Xn'], p['G'], a0, L0, rho=p['rho'], y=p['yn']))
        eng.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_training_state_survives(dtype):
    from scfgp_amd.engine import HipEngine
    D, S, M = 20, 20, 280
    params = synth.make_params(7, D, S, M, abc=(-1.0, 0.0, -1.0))
    X = synth.make_X(7, 1500, D)
    y = np.sin(3 * X[:, :1]) + 0.1 * synth.normal(10, 0, 1500)[:, None]
    Xn = synth.make_X(9, 3200, D); yn = np.sin(3 * Xn[:, 0]); Gn = 3 * np.cos(3 * Xn[:, :1]) * np.eye(D)[:1]   # 21 rows a point: 3 chunks
    eng = HipEngine(D, S, M, dtype=dtype); eng.set_params(params); eng.set_data(X, y)
    c0, g0, a0, L0 = eng.eval(want_grad=True)
    c0, g0, a0, L0 = float(c0), g0.copy(), a0.copy(), L0.copy()
    eng.condition_grad(Xn, Gn, a0, L0, y=yn)
    eng.condition_grad(Xn[:7], Gn[:7, [4, 0]], a0, L0, dims=[4, 0])
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
            eng.condition_grad(Xn[:500], Gn[:500], al, Li, y=yn[:500])
        h2, al2, Li2 = eng.train(3)
        runs.append((h1.copy(), h2.copy(), eng.get_params().copy(), al2.copy(), Li2.copy()))
        eng.close()
    for u, v in zip(*runs):
        assert np.array_equal(u, v)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_the_entry_points_that_share_its_buffers_follow_it_correctly(dtype):
    """predict, predict_gradcov and condition read the chunk buffers that the call has just filled with observation rows: each gives the
    bits it gives on a fresh context"""
    shape = R.SHAPES[5]
    D, S, M, N0, n, dims = shape
    p, a0, L0 = _case(*shape)
    X = p['X0'][:700]

    def followers(eng):
        mu, sd = eng.predict(X, a0, L0)
        gc = eng.predict_gradcov(X[:300], a0, L0, want=('dmu', 'dvar', 'asub'))
        al, Li = eng.condition(X, p['y0'][:700], a0, L0)
        return mu, sd, gc['dmu'], gc['dvar'], gc['asub'], al, Li
    eng = _engine(D, S, M, dtype, p['params'])
    fresh = followers(eng)
    eng.close()
    eng = _engine(D, S, M, dtype, p['params'])
    eng.condition_grad(p['Xn'], p['G'], a0, L0, rho=p['rho'], y=p['yn'])
    after = followers(eng)
    eng.close()
    for u, v in zip(fresh, after):
        assert np.array_equal(u, v)


@pytest.mark.parametrize('xalgo', Scaler.algos)
def test_raw_mode_equals_scaled_mode(xalgo):
    """psi_raw = g psi and the target is the same G, so the raw call is the scaled call with G / g and rho g^2 (g > 0): both are fp64
    evaluations of the same element-wise formulas, and the update that follows is the same code on inputs that close (the 1e-12 of
    tests/test_gpu_condition.py's test of the same name)"""
    from scfgp_amd.engine import HipEngine
    q = R.raw_problem(xalgo)
    D, S, M = q['D'], q['S'], q['M']
    xs, cols = q['xs'], q['xs'].data['cols']
    eng = HipEngine(D, S, M, dtype='f64'); eng.set_params(q['params']); eng.set_x_scaler(xs)
    Xr = q['Xr']
    fx = np.ascontiguousarray(xs.forward_transform(Xr)); g = xs.forward_derivative(Xr)
    assert Xr.shape[1] == 4 and fx.shape[1] == 3 and np.all(g > 0)                  # the constant column is dropped
    Gs = q['dY'] * q['ys'].forward_derivative(q['yr'])                              # scaled target per raw input, 4 columns
    ysc = q['ys'].forward_transform(q['yr'])
    for rho in (None, q['rho']):
        for y in (None, ysc):
            ar, Lr = eng.condition_grad(Xr, Gs, q['alpha'], q['Li'], rho=rho, y=y, raw=True)
            rs = (1.0 if rho is None else rho[:, cols]) * g ** 2
            a0, L0 = eng.condition_grad(fx, Gs[:, cols] / g, q['alpha'], q['Li'], rho=rs, y=y)
            assert rel(ar, a0) < 1e-12 and rel(Lr, L0) < 1e-12
            assert rel(a0, q['alpha']) > 1e-6                                       # the observations did move the posterior
    # a subset of raw columns that names the dropped one: its entries are ignored
    ar, Lr = eng.condition_grad(Xr, Gs[:, [3, 2, 0]], q['alpha'], q['Li'], dims=[3, 2, 0], raw=True)
    a0, L0 = eng.condition_grad(fx, Gs[:, [3, 0]] / g[:, [2, 0]], q['alpha'], q['Li'], dims=[2, 0], rho=g[:, [2, 0]] ** 2)
    assert rel(ar, a0) < 1e-12 and rel(Lr, L0) < 1e-12
    eng.close()


def _fitted_model(y_scaling, tmp_path):
    from scfgp_amd import SCFGP
    rng = np.random.default_rng(5)
    np.random.seed(5)
    X = rng.uniform(-2, 2, (400, 3))
    X = np.column_stack([X[:, :2], np.full(400, 4.0), X[:, 2:]])     # a constant column
    y = 3.0 + np.sin(X[:, :1]) + 0.5 * X[:, 1:2] ** 2 + 0.05 * rng.standard_normal((400, 1))
    dY = np.column_stack([np.cos(X[:, 0]), X[:, 1], np.full(400, 9.0), np.zeros(400)])
    model = SCFGP(sparsity=3, nfeats=12, device_scaler=True, y_scaling_method=y_scaling)
    model.fit(X[:240], y[:240], max_iter=10,
              algo={'algo': 'adam', 'algo_params': {'learning_rate': 0.02, 'beta1': 0.9, 'beta2': 0.999, 'epsilon': 1e-8}})
    path = str(tmp_path / 'model.npz')
    model.save(path)
    fresh = SCFGP(sparsity=3, nfeats=12, device_scaler=True, y_scaling_method=y_scaling)
    fresh.load(path)                                                   # never saw set_data: no rows
    return fresh, X[240:340], y[240:340], dY[240:340]


def test_facade_on_a_restored_checkpoint(tmp_path):
    fresh, X, y, dY = _fitted_model('normal', tmp_path)
    assert fresh.X is None and fresh.y_scaler.affine
    a_old, L_old = np.array(fresh.alpha), np.array(fresh.Li)
    owner = fresh._owner('test')
    rng = np.random.default_rng(1)
    rho = rng.choice(R.RHO_VALUES, size=dY.shape)
    sy = float(np.asarray(fresh.y_scaler.data['std']).reshape(-1)[0])
    for kw, eng_kw in ((dict(), dict()),
                       (dict(y=y, rho=rho), dict(rho=rho, y=fresh.y_scaler.forward_transform(y))),
                       (dict(dims=[1, 2, 0]), dict(dims=[1, 2, 0]))):
        fresh.alpha, fresh.Li = a_old.copy(), L_old.copy()
        d = dY if 'dims' not in kw else dY[:, kw['dims']]
        assert fresh.condition_grad(X, d, **kw) is fresh
        assert fresh.X is None and not np.array_equal(fresh.alpha, a_old)
        a1, L1 = owner.engine.condition_grad(X, d / sy, a_old, L_old, raw=True, **eng_kw)      # the host's conversion: d y~ / d y = 1 / std
        assert rel(fresh.alpha, a1) < 1e-12 and rel(fresh.Li, L1) < 1e-12
    mu, sd = fresh.predict(X)[:2]
    assert np.all(np.isfinite(mu)) and np.all(np.isfinite(sd))


def test_facade_needs_y_where_the_y_scaler_is_not_affine(tmp_path):
    fresh, X, y, dY = _fitted_model('auto-normal', tmp_path)
    a_old = np.array(fresh.alpha)
    with pytest.raises(ValueError, match='not affine'):
        fresh.condition_grad(X, dY)
    assert np.array_equal(fresh.alpha, a_old)
    L_old = np.array(fresh.Li)
    fresh.condition_grad(X, dY, y=y)
    a1, L1 = fresh._owner('test').engine.condition_grad(X, dY * fresh.y_scaler.forward_derivative(y), a_old, L_old, raw=True,
                                                        y=fresh.y_scaler.forward_transform(y))
    assert rel(fresh.alpha, a1) < 1e-12 and rel(fresh.Li, L1) < 1e-12 and not np.array_equal(fresh.alpha, a_old)


def test_errors():
    import ctypes as C
    from scfgp_amd.engine import HipEngine
    from scfgp_amd._lib import dptr
    shape = R.SHAPES[1]
    D, S, M, N0, n, dims = shape
    p, a0, L0 = _case(*shape)
    ref = _reference(shape, True, 'drawn')
    eng = _engine(D, S, M, 'f64', p['params'])
    X = np.ascontiguousarray(p['Xn']); G = np.ascontiguousarray(p['G']); rho = np.ascontiguousarray(p['rho']); y = np.ascontiguousarray(p['yn'])
    a = np.ascontiguousarray(a0).ravel()
    ao = np.full(a.size, 3.0); Lo = np.full(L0.shape, 3.0)
    keep = []

    def ip(v):
        keep.append(np.array(v, dtype=np.int32))
        return keep[-1].ctypes.data_as(C.POINTER(C.c_int32))

    def lib_call(X_=X, n_=n, dims_=None, nd_=D, G_=G, rho_=rho, y_=y, a_=a, L_=L0, mode=0, ao_=ao, Lo_=Lo):
        eng._check_undelivered(eng.lib.scfgp_condition_grad(eng.ctx, dptr(X_), n_, dims_, nd_, dptr(G_), dptr(rho_), dptr(y_), dptr(a_),
                                                            dptr(L_), mode, dptr(ao_), dptr(Lo_)), 'condition_grad')
    refusals = [(dict(X_=None), 'condition_grad: bad arguments'), (dict(G_=None), 'condition_grad: bad arguments'),
                (dict(a_=None), 'condition_grad: bad arguments'), (dict(L_=None), 'condition_grad: bad arguments'),
                (dict(ao_=None), 'condition_grad: bad arguments'), (dict(Lo_=None), 'condition_grad: bad arguments'),
                (dict(n_=0), 'condition_grad: n must be at least 1'),
                (dict(nd_=0), 'condition_grad: nd must lie in 1..D'), (dict(nd_=D + 1), 'condition_grad: nd must lie in 1..D'),
                (dict(nd_=D - 1), 'condition_grad: dims == NULL needs nd == D'),
                (dict(dims_=ip([0, 1, D]), nd_=3), r'condition_grad: dims\[2\] is out of range or repeated'),
                (dict(dims_=ip([0, -1, 2]), nd_=3), r'condition_grad: dims\[1\] is out of range or repeated'),
                (dict(dims_=ip([2, 0, 1, 0]), nd_=4), r'condition_grad: dims\[3\] is out of range or repeated'),
                (dict(mode=2), 'condition_grad: bad mode'), (dict(mode=-1), 'condition_grad: bad mode'),
                (dict(mode=1), 'condition_grad: no X scaler set')]
    rb = rho.copy(); rb[2, 1] = np.nan; rb[4, 3] = -1.0                  # the negative entry is reported though it stands behind the NaN
    refusals.append((dict(rho_=rb), r'condition_grad: rho\[4, 3\] is negative'))
    refusals.append((dict(rho_=np.zeros_like(rho), y_=None), 'condition_grad: every rho is zero and no values are given'))
    for kw, text in refusals:
        with pytest.raises(ValueError, match=text):
            lib_call(**kw)
    nonfinite = []
    for bad in (np.nan, np.inf):
        rb = rho.copy(); rb[2, 1] = bad
        nonfinite.append((dict(rho_=rb), r'rho\[2, 1\] is not finite'))
        Gb = G.copy(); Gb[np.argwhere(rho > 0)[5][0], np.argwhere(rho > 0)[5][1]] = bad
        nonfinite.append((dict(G_=Gb), 'non-finite rows, observations or factors'))
        yb = y.copy(); yb[17] = bad
        nonfinite.append((dict(y_=yb), 'non-finite'))
    Xb = X.copy(); Xb[3, 2] = np.nan
    nonfinite.append((dict(X_=Xb), 'non-finite'))
    Lb = L0.copy(); Lb[50, 3] = np.inf
    nonfinite.append((dict(L_=Lb), 'non-finite'))
    ab = a.copy(); ab[5] = np.nan
    nonfinite.append((dict(a_=ab), 'non-finite'))
    for kw, text in nonfinite:
        with pytest.raises(FloatingPointError, match=text):
            lib_call(**kw)
    # SCFGP_ENOTPD: S = I + C^T C is positive definite in exact arithmetic, so only a precision beyond what fp64 absorbs loses the
    # factor: one point with rho = 1e100 makes S = I + 1e100 (rank 5), whose Schur complements drown the identity in rounding noise.  The
    # failed factorisation leaves NaN behind, which the finite check of the stage's results reports first, as in scfgp_condition whose
    # finish this is: the call is refused as non-finite (measured), and SCFGP_ENOTPD stays for a pivot that fails without a NaN
    with pytest.raises((np.linalg.LinAlgError, FloatingPointError), match='not positive definite|non-finite'):
        eng._check(eng.lib.scfgp_condition_grad(eng.ctx, dptr(X), 1, None, D, dptr(G), dptr(np.full((1, D), 1e100)), None, dptr(a), dptr(L0), 0,
                                                dptr(ao), dptr(Lo)), 'condition_grad')
    assert np.all(ao == 3.0) and np.all(Lo == 3.0)                       # the outputs are untouched by every failure
    mu, sd = eng.predict(p['Xs'], a0, L0)                                # a correct predict follows
    mu0, sd0 = O.predict(p['Xs'], a0, L0, p['params'], S, M)
    parity.check_predict(mu, sd, mu0, sd0, 'f64')
    with pytest.raises(ValueError, match='columns'):
        eng.condition_grad(X[:, :4], G, a0, L0)
    with pytest.raises(ValueError, match='one column per observed input'):
        eng.condition_grad(X, G[:, :-1], a0, L0)
    with pytest.raises(ValueError, match='one column per observed input'):
        eng.condition_grad(X, G, a0, L0, rho=rho[:-1])
    with pytest.raises(ValueError, match='entries'):
        eng.condition_grad(X, G, a0, L0, y=y[:-1])
    with pytest.raises(ValueError, match='shape'):
        eng.condition_grad(X, G, a0, L0[:-1])
    with pytest.raises(ValueError, match='scaler'):
        eng.condition_grad(X, G, a0, L0, raw=True)
    al, Li = eng.condition_grad(X, G, a0, L0, rho=rho, y=y)              # the context still works
    _checks(eng, al, Li, ref, p['Xs'], 'f64', 'after the errors')
    eng.close()
    fresh = HipEngine(D, S, M, dtype='f64')                              # no parameters yet
    with pytest.raises(ValueError, match='parameters not set'):
        fresh.condition_grad(X, G, a0, L0)
    fresh.close()
