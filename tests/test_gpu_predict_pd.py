"""GPU tier of the partial-dependence and ICE curves (pd.hip: scfgp_predict_pd): parity with the numpy brute force over the expanded rows
(tests/pd_ref.py) over the geometry classes, a three-chunk call, the bit-level promises of include/scfgp_hip.h, the documented bounds
of G and ndim, self-consistency against predict / acquire / ice, raw mode through every X scaler, the refusals, the training state and
the SCFGP facade (partial_dependence).  Every geometry of the parity tests has K <= 172: the 128-wide column plan of K > 256, K = 256 =
Kp, the factors of a real fit and a context that other entry points share are covered by the geometry sweep and the stale-state
sequences (tests/test_gpu_posterior_geometry.py, tests/test_gpu_posterior_sequence.py)."""
import ctypes
import itertools

import numpy as np
import pytest

from scfgp_amd import synth
from scfgp_amd._lib import dptr
from scfgp_amd.scaler import Scaler
from tests import gradcov_ref as GR
from tests import pd_ref as R

pytestmark = pytest.mark.gpu

# pd, sd, cov: BOUNDS of tests/test_gpu_predict_cov.py -- the factor comes from the same apply_c and enters the same bilinear form.
# ice: BOUNDS of tests/test_gpu_sample.py -- it is the same product.
BOUNDS = {'f64': 1e-10, 'f32': 6e-6}
BOUNDS_ICE = {'f64': 1e-10, 'f32': 3e-6}
ALL = ('pd', 'sd', 'cov', 'ice')


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def _engine(D, S, M, dtype):
    from scfgp_amd.engine import HipEngine
    params, alpha, Li = R.synthetic(D, S, M)
    eng = HipEngine(D, S, M, dtype=dtype); eng.set_params(params)
    return eng, params, alpha, Li


def _errors(out, ref, dtype, what):
    """relative errors of the outputs present against the reference tuple (pd, sd, cov, ice, ..), printed, then asserted"""
    errs = {k: rel(out[k], ref[i]) for i, k in enumerate(ALL) if k in out}
    frac = {k: errs[k] / (BOUNDS_ICE if k == 'ice' else BOUNDS)[dtype] for k in errs}
    print(what, dtype, ' '.join('%s=%.2e (%.3f of its bound)' % (k, errs[k], frac[k]) for k in errs))
    assert max(frac.values()) < 1.0, errs
    return errs


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('D,S,M', R.GEOMETRIES)
def test_parity_over_the_geometry_classes(D, S, M, dtype):
    eng, params, alpha, Li = _engine(D, S, M, dtype)
    Xs = R.points(D)
    T, G = len(Xs), 9
    w = 0.25 + synth.uniform(77, 0, T)
    dims = R.dims_for(D)
    grid = R.make_grid(Xs, dims, G)
    out = eng.predict_pd(Xs, alpha, Li, dims, grid, w=w, want=ALL)
    nd = len(dims)
    assert out['pd'].shape == (nd, G) and out['sd'].shape == (nd, G) and out['cov'].shape == (nd, G, G) and out['ice'].shape == (nd, T, G)
    ref = R.brute(Xs, w, alpha, Li, params, S, M, dims, grid)
    _errors(out, ref, dtype, 'parity T=%d %s' % (T, (D, S, M)))
    assert np.all(out['sd'] >= 0)
    diag = np.diagonal(out['cov'], axis1=1, axis2=2)
    print('diag(cov) against sd^2: %.2e' % rel(diag, out['sd'] ** 2))
    assert rel(diag, out['sd'] ** 2) < (1e-10 if dtype == 'f64' else BOUNDS['f32'])
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_three_chunks_parity_repeatability_zero_weights_and_ice_rows(dtype):
    D, S, M = 7, 12, 3
    eng, params, alpha, Li = _engine(D, S, M, dtype)
    T, G = 2 * 32768 + 300, 5
    Xs = synth.make_X(505, T, D)
    w = 0.25 + synth.uniform(82, 0, T)
    dims = list(range(D))
    grid = R.make_grid(Xs, dims, G)
    out = eng.predict_pd(Xs, alpha, Li, dims, grid, w=w, want=ALL)
    ref = R.brute(Xs, w, alpha, Li, params, S, M, dims, grid, want_ice=False)
    _errors({k: out[k] for k in ('pd', 'sd', 'cov')}, ref, dtype, 'three chunks T=%d' % T)
    again = eng.predict_pd(Xs, alpha, Li, dims, grid, w=w, want=('pd', 'sd', 'cov'))
    for k in again:
        assert np.array_equal(again[k], out[k]), k
    # trailing rows of weight zero, one of them not finite, change nothing (promise 6)
    extra = synth.make_X(506, 5, D); extra[2, 3] = np.nan
    tail = eng.predict_pd(np.vstack([Xs, extra]), alpha, Li, dims, grid, w=np.r_[w, np.zeros(5)], want=('pd', 'sd', 'cov'))
    for k in tail:
        assert np.array_equal(tail[k], out[k]), k
    # the ice rows around the chunk boundaries equal a call on that row alone, bit for bit (promise 5)
    for t in (32767, 32768, 65536):
        one = eng.predict_pd(Xs[t:t + 1], alpha, Li, dims, grid, want=('ice',))['ice']
        assert np.array_equal(one[:, 0, :], out['ice'][:, t, :]), t
    sel = np.r_[0:4, 32766:32770, 65534:65538, T - 2:T]
    ice = R.closed(Xs[sel], None, alpha, Li, params, S, M, dims, grid)[3]
    e = rel(out['ice'][:, sel, :], ice)
    print('three chunks ice', dtype, '%.2e' % e)
    assert e < BOUNDS_ICE[dtype]
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('D,S,M', [(15, 15, 60), (70, 5, 60)])
def test_bit_level_promises(D, S, M, dtype):
    eng, params, alpha, Li = _engine(D, S, M, dtype)
    Xs = R.points(D)
    T, G = len(Xs), 9
    w = 0.25 + synth.uniform(79, 0, T)
    dims = [0, D // 2, D - 1, 3]
    grid = R.make_grid(Xs, dims, G)
    full = eng.predict_pd(Xs, alpha, Li, dims, grid, w=w, want=ALL)
    # 2: the other dimensions of the call and their order do not matter
    pick = [2, 0]
    part = eng.predict_pd(Xs, alpha, Li, [dims[a] for a in pick], grid[pick], w=w, want=ALL)
    for k in ALL:
        assert np.array_equal(part[k], full[k][pick]), k
    # 3: an entry depends on its own grid value(s) alone: a shorter, permuted grid
    perm = [7, 2, 5, 0]
    short = eng.predict_pd(Xs, alpha, Li, dims, grid[:, perm], w=w, want=ALL)
    assert np.array_equal(short['pd'], full['pd'][:, perm]) and np.array_equal(short['sd'], full['sd'][:, perm])
    assert np.array_equal(short['ice'], full['ice'][:, :, perm])
    assert np.array_equal(short['cov'], full['cov'][:, perm][:, :, perm])
    # 4: symmetric bit for bit
    assert np.array_equal(full['cov'], full['cov'].transpose(0, 2, 1))
    # 7: every combination of outputs
    for r in (1, 2, 3):
        for want in itertools.combinations(ALL, r):
            out = eng.predict_pd(Xs, alpha, Li, dims, grid, w=w, want=want)
            assert sorted(out) == sorted(want)
            for k in want:
                assert np.array_equal(out[k], full[k]), (want, k)
    # 5: w does not enter ice
    assert np.array_equal(eng.predict_pd(Xs, alpha, Li, dims, grid, want=('ice',))['ice'], full['ice'])
    eng.close()


def test_f16x3_context_equals_fp32_context():
    from scfgp_amd.engine import HipEngine
    for D, S, M in ((15, 15, 60), (70, 5, 60)):
        e32, params, alpha, Li = _engine(D, S, M, 'f32')
        e16 = HipEngine(D, S, M, dtype='f16x3'); e16.set_params(params)
        Xs = R.points(D)
        dims = [0, D - 1]
        grid = R.make_grid(Xs, dims, 6)
        w = 0.25 + synth.uniform(80, 0, len(Xs))
        a = e32.predict_pd(Xs, alpha, Li, dims, grid, w=w, want=ALL)
        b = e16.predict_pd(Xs, alpha, Li, dims, grid, w=w, want=ALL)
        for k in ALL:
            assert np.array_equal(a[k], b[k]), k
        e32.close(); e16.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('G', [1, 1024])
def test_the_bounds_of_the_grid(G, dtype):
    D, S, M = 7, 12, 3
    eng, params, alpha, Li = _engine(D, S, M, dtype)
    T = 300
    Xs = synth.make_X(606, T, D)
    w = 0.25 + synth.uniform(83, 0, T)
    dims = list(range(D))
    grid = R.make_grid(Xs, dims, G)
    out = eng.predict_pd(Xs, alpha, Li, dims, grid, w=w, want=ALL)
    ref = R.brute(Xs, w, alpha, Li, params, S, M, dims, grid)
    _errors(out, ref, dtype, 'G=%d' % G)
    assert np.array_equal(out['cov'], out['cov'].transpose(0, 2, 1))
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_every_dimension_of_a_wide_input(dtype):
    """ndim = D = 70: the dimension groups of the block records and of the stacked mean rows"""
    D, S, M = 70, 5, 60
    eng, params, alpha, Li = _engine(D, S, M, dtype)
    Xs = R.points(D)
    w = 0.25 + synth.uniform(84, 0, len(Xs))
    dims = list(range(D))[::-1]
    grid = R.make_grid(Xs, dims, 3)
    out = eng.predict_pd(Xs, alpha, Li, dims, grid, w=w, want=ALL)
    ref = R.brute(Xs, w, alpha, Li, params, S, M, dims, grid)
    _errors(out, ref, dtype, 'ndim=70')
    # At this K both budgets (64 MiB of block records, 32 768 stacked rows) hold all 70 dimensions in one group.  The option caps a
    # group at 16 dimensions, so the sums and the curves each take five groups, the last one ragged: the same bits (promise 2).
    eng.set_option('test_pd_group', 16)
    grouped = eng.predict_pd(Xs, alpha, Li, dims, grid, w=w, want=ALL)
    eng.set_option('test_pd_group', 0)
    for k in ALL:
        assert np.array_equal(grouped[k], out[k]), k
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_self_consistency_without_the_reference(dtype):
    D, S, M = 15, 15, 60
    eng, params, alpha, Li = _engine(D, S, M, dtype)
    Xs = R.points(D)
    dims = [1, 8, 14]
    G = 7
    grid = R.make_grid(Xs, dims, G)
    # T = 1: the PD curve is the prediction at the replaced rows, its sd the latent sd there
    one = eng.predict_pd(Xs[5:6], alpha, Li, dims, grid, want=('pd', 'sd', 'ice'))
    for a, d in enumerate(dims):
        Xe = np.repeat(Xs[5:6], G, 0); Xe[:, d] = grid[a]
        mu = eng.predict(Xe, alpha, Li)[0].ravel()
        sd = eng.acquire(Xe, alpha, Li, 'ucb', beta=1.0, noise=False, want=('acq', 'sd'))['sd']
        e = (rel(one['pd'][a], mu), rel(one['ice'][a, 0], mu), rel(one['sd'][a], sd))
        print('T=1', dtype, 'dimension %d: pd %.2e ice %.2e sd %.2e' % ((d,) + e))
        assert e[0] < BOUNDS[dtype] and e[1] < BOUNDS_ICE[dtype] and e[2] < BOUNDS[dtype]
    # pd is the weighted mean of the ICE curves
    w = 0.25 + synth.uniform(85, 0, len(Xs))
    out = eng.predict_pd(Xs, alpha, Li, dims, grid, w=w, want=('pd', 'ice'))
    e = rel(out['pd'], np.einsum('t,atg->ag', w / w.sum(), out['ice']))
    print('pd against the weighted mean of ice', dtype, '%.2e' % e)
    assert e < BOUNDS_ICE[dtype]
    eng.close()


def _scaled_grid(xs, Xr, cols, grid):
    """the X scaler's forward transform of the grid values of raw column cols[a], on the host"""
    out = np.empty_like(grid)
    kept = list(xs.data['cols'])
    for a, cc in enumerate(cols):
        fake = np.repeat(Xr[:1], grid.shape[1], 0); fake[:, cc] = grid[a]
        out[a] = xs.forward_transform(fake)[:, kept.index(cc)]
    return out


@pytest.mark.parametrize('xalgo', Scaler.algos)
def test_raw_mode_through_every_x_scaler(xalgo):
    from scfgp_amd.engine import HipEngine
    (D, S, M), xs, (params, alpha, Li), Xr = GR.raw_problem(xalgo)
    eng = HipEngine(D, S, M, dtype='f64'); eng.set_params(params); eng.set_x_scaler(xs)
    T = len(Xr)
    w = 0.25 + synth.uniform(81, 0, T)
    cols = [3, 0, 1]                                              # raw columns; column 2 is constant and dropped by the scaler
    grid = R.make_grid(Xr, cols, 6)
    # Six values in and a little around the rows' range, then two that lie three spans outside it and so outside the range the scaler
    # was fitted on (below its minimum: the sign branch of the Box-Cox map): the device's transform of the grid is the scaler's own
    # formula there too.
    lo, hi = Xr[:, cols].min(0), Xr[:, cols].max(0)
    grid = np.column_stack([grid, lo - 3.0 * (hi - lo), hi + 3.0 * (hi - lo)])
    raw = eng.predict_pd(Xr, alpha, Li, cols, grid, w=w, mode='raw', want=ALL)
    kept = list(xs.data['cols'])
    Xsc = np.ascontiguousarray(xs.forward_transform(Xr))
    gsc = _scaled_grid(xs, Xr, cols, grid)
    sc = eng.predict_pd(Xsc, alpha, Li, [kept.index(cc) for cc in cols], gsc, w=w, want=ALL)
    for k in ALL:
        e = rel(raw[k], sc[k])
        print(xalgo, k, '%.2e' % e)
        assert e < 1e-12, k
    ref = R.brute(Xsc, w, alpha, Li, params, S, M, [kept.index(cc) for cc in cols], gsc)
    _errors(raw, ref, 'f64', 'raw mode %s' % xalgo)
    with pytest.raises(ValueError, match='dropped'):
        eng.predict_pd(Xr, alpha, Li, [2], grid[:1], mode='raw')
    eng.close()


def test_refusals_leave_the_outputs_untouched_and_the_context_working():
    from scfgp_amd.engine import HipEngine
    D, S, M = 5, 4, 60
    eng, params, alpha, Li = _engine(D, S, M, 'f64')
    T, G, nd = 10, 4, 2
    Xs = synth.make_X(3, T, D)
    grid = R.make_grid(Xs, [1, 4], G)
    dims = (ctypes.c_int * 2)(1, 4)
    bufs = [np.full((nd, G), 7.0), np.full((nd, G), 7.0), np.full((nd, G, G), 7.0), np.full((nd, T, G), 7.0)]
    o = [dptr(b) for b in bufs]
    fn = eng.lib.scfgp_predict_pd
    A, L, X, Gr = dptr(alpha), dptr(Li), dptr(Xs), dptr(grid)

    def refused(rc, match, *args):
        assert fn(eng.ctx, *args) == rc
        assert match in eng.last_error(), eng.last_error()
        assert all(np.all(b == 7.0) for b in bufs)

    refused(-1, 'bad arguments', None, T, None, A, L, dims, nd, Gr, G, 0, *o)
    refused(-1, 'bad arguments', X, T, None, None, L, dims, nd, Gr, G, 0, *o)
    refused(-1, 'bad arguments', X, T, None, A, None, dims, nd, Gr, G, 0, *o)
    refused(-1, 'bad arguments', X, T, None, A, L, None, nd, Gr, G, 0, *o)
    refused(-1, 'bad arguments', X, T, None, A, L, dims, nd, None, G, 0, *o)
    refused(-1, 'no output', X, T, None, A, L, dims, nd, Gr, G, 0, None, None, None, None)
    refused(-1, 'T must', X, 0, None, A, L, dims, nd, Gr, G, 0, *o)
    refused(-1, 'G must', X, T, None, A, L, dims, nd, Gr, 0, 0, *o)
    refused(-1, 'G must', X, T, None, A, L, dims, nd, Gr, 1025, 0, *o)
    refused(-1, 'ndim must', X, T, None, A, L, dims, 0, Gr, G, 0, *o)
    refused(-1, 'ndim must', X, T, None, A, L, dims, D + 1, Gr, G, 0, *o)
    refused(-1, 'out of range', X, T, None, A, L, (ctypes.c_int * 2)(1, D), nd, Gr, G, 0, *o)
    refused(-1, 'out of range', X, T, None, A, L, (ctypes.c_int * 2)(-1, 2), nd, Gr, G, 0, *o)
    refused(-1, 'given twice', X, T, None, A, L, (ctypes.c_int * 2)(4, 4), nd, Gr, G, 0, *o)
    refused(-1, 'bad mode', X, T, None, A, L, dims, nd, Gr, G, 2, *o)
    refused(-1, 'bad mode', X, T, None, A, L, dims, nd, Gr, G, -1, *o)
    refused(-1, 'no X scaler', X, T, None, A, L, dims, nd, Gr, G, 1, *o)
    w = np.ones(T)
    wb = w.copy(); wb[T - 1] = -1e-300
    refused(-1, 'negative weight at row 9', X, T, dptr(wb), A, L, dims, nd, Gr, G, 0, *o)
    refused(-1, 'positive weight', X, T, dptr(np.zeros(T)), A, L, dims, nd, Gr, G, 0, *o)
    for bad in (np.nan, np.inf):
        wb = w.copy(); wb[3] = bad
        refused(-4, 'non-finite weights', X, T, dptr(wb), A, L, dims, nd, Gr, G, 0, *o)
        gb = grid.copy(); gb[1, 2] = bad
        refused(-4, 'non-finite grid', X, T, None, A, L, dims, nd, dptr(gb), G, 0, *o)
    Xb = Xs.copy(); Xb[4, 0] = np.nan                             # a live row that is not finite: the weighted sum is not
    refused(-4, 'non-finite weighted sum', dptr(Xb), T, None, A, L, dims, nd, Gr, G, 0, *o)
    # ... unless its weight is zero: then it only has no finite ice row
    wz = w.copy(); wz[4] = 0.0
    assert fn(eng.ctx, dptr(Xb), T, dptr(wz), A, L, dims, nd, Gr, G, 0, *o) == 0
    assert np.all(np.isfinite(bufs[0])) and np.all(np.isfinite(bufs[1])) and np.all(np.isfinite(bufs[2]))
    assert np.all(np.isnan(bufs[3][:, 4, :])) and np.all(np.isfinite(np.delete(bufs[3], 4, axis=1)))
    # a good call succeeds afterwards
    ref = R.brute(Xs, None, alpha, Li, params, S, M, [1, 4], grid)
    _errors(eng.predict_pd(Xs, alpha, Li, [1, 4], grid, want=ALL), ref, 'f64', 'after the refusals')
    with pytest.raises(ValueError):
        eng.predict_pd(Xs, alpha, Li, [1, 4], grid, mode='y')      # no raw-y mode
    with pytest.raises(ValueError):
        eng.predict_pd(Xs, alpha, Li, [1, 4], grid, want=())
    with pytest.raises(ValueError, match='scaler'):
        eng.predict_pd(Xs, alpha, Li, [1, 4], grid, mode='raw')
    with pytest.raises(FloatingPointError):
        eng.predict_pd(Xb, alpha, Li, [1, 4], grid)
    eng.close()
    # a non-finite grid value after the X scaler's transform (raw mode)
    (D, S, M), xs, (params, alpha, Li), Xr = GR.raw_problem('normal')
    eng = HipEngine(D, S, M, dtype='f64'); eng.set_params(params); eng.set_x_scaler(xs)
    g = np.array([[1.0, np.nan, 2.0]])
    with pytest.raises(FloatingPointError, match='grid'):
        eng.predict_pd(Xr, alpha, Li, [0], g, mode='raw')
    assert np.all(np.isfinite(eng.predict_pd(Xr, alpha, Li, [0], np.array([[1.0, 1.5, 2.0]]), mode='raw')['pd']))
    eng.close()
    fresh = HipEngine(5, 4, 60, dtype='f64')                       # no parameters yet
    with pytest.raises(ValueError, match='parameters not set'):
        fresh.predict_pd(Xs, np.zeros(128), np.eye(128), [1, 4], grid)
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
    Xs = synth.make_X(9, 33000, D)
    p0 = eng.predict(Xs, a0, L0)
    dims = [0, 7, 19]
    out = eng.predict_pd(Xs, a0, L0, dims, R.make_grid(Xs, dims, 5), w=0.25 + synth.uniform(86, 0, len(Xs)), want=ALL)
    assert all(np.all(np.isfinite(out[k])) for k in ALL)
    c1, g1, a1, L1 = eng.eval(want_grad=True)
    assert float(c1) == c0 and np.array_equal(g1, g0) and np.array_equal(a1, a0) and np.array_equal(L1, L0)
    for u, v in zip(eng.predict(Xs, a0, L0), p0):
        assert np.array_equal(u, v)
    eng.close()


def test_facade_partial_dependence():
    """A target that depends on its first input only: that input's importance dominates, and the flat input's curve stays within three
    of its own posterior standard deviations of its mean."""
    from scfgp_amd import SCFGP
    rng = np.random.default_rng(12)
    np.random.seed(12)
    N = 500
    X = rng.uniform(-2, 2, (N, 2))
    y = np.sin(1.5 * X[:, :1]) + 0.05 * rng.standard_normal((N, 1))
    model = SCFGP(sparsity=2, nfeats=20, device_scaler=True)
    n = N * 4 // 5
    model.set_data(X[:n], y[:n])
    model.optimize(X[n:], y[n:], max_iter=100,
                   algo={'algo': 'adam', 'algo_params': {'learning_rate': 0.02, 'beta1': 0.9, 'beta2': 0.999, 'epsilon': 1e-8}})
    res = model.partial_dependence(X, grid=12, ice=True, cov=True)
    assert list(res['dims']) == [0, 1]
    assert res['grid'].shape == (2, 12) and res['pd'].shape == (2, 12) and res['sd'].shape == (2, 12)
    assert res['cov'].shape == (2, 12, 12) and res['ice'].shape == (2, N, 12) and res['importance'].shape == (2,)
    assert np.array_equal(res['importance'], res['pd'].std(axis=1))
    dev = np.abs(res['pd'][1] - res['pd'][1].mean()) / res['sd'][1]
    print('importance', res['importance'], 'flat input: largest deviation from its mean %.2f sd' % dev.max())
    assert res['importance'][0] > 3 * res['importance'][1]
    assert np.all(dev <= 3.0)
    # the engine's raw mode is what the facade calls, and explicit grids and a subset of the dimensions are accepted
    eng = model.pred_func.__self__.engine
    out = eng.predict_pd(X, model.alpha, model.Li, [0, 1], res['grid'], mode='raw', want=ALL)
    for k in ALL:
        assert np.array_equal(out[k], res[k]), k
    one = model.partial_dependence(X, dims=[1], grid=res['grid'][1], weights=np.ones(N))
    assert np.array_equal(one['pd'][0], res['pd'][1]) and np.array_equal(one['sd'][0], res['sd'][1])
    other = SCFGP(sparsity=2, nfeats=20)
    other.pred_func = lambda Xs, alpha, Li: None
    with pytest.raises(TypeError):
        other.partial_dependence(X)
