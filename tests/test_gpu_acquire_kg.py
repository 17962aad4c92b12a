"""GPU tier of scfgp_acquire_kg (kg.hip): the node table bit for bit against the numpy restatement (tests/kg_ref.py) fed the device's own
predict_cov, predict and sigma; kg / kg_hi against the restatement's sums at the device's own table; the bracket around the exact
knowledge gradient of numpy features, with a Lipschitz slack computed in the test; position, chunk, permutation, duplication and
column-split independence bit for bit; one reference row; the argmax rule; every error with untouched outputs; the survival of the
training state; the SCFGP facade.

Measured on the device (MI355X), values against tests/kg_ref.py's sums at the device's table in the measure max |delta| / max kg_hi,
worst over shapes, dtypes, noise, directions and node sets: 7.1e-16 (the bound is 8 x MEASURED_KG_ERR = 8.0e-15)."""
import ctypes as C

import numpy as np
import pytest

from oracle import scfgp_oracle as O
from scfgp_amd import synth
from tests import kg_ref as G
from tests import pred_cov_ref as PC

pytestmark = pytest.mark.gpu

# (D, S, M, T, R): K = 42, 128, 600; no size is a multiple of 16 or 128, the k loop ends on a ragged tile, K = 600 crosses the fp32 flush
SHAPES = [(3, 1, 20, 301, 157), (5, 4, 60, 129, 257), (20, 20, 280, 130, 391)]
# only fp64 arithmetic through other libm implementations differs: the margin tests/test_gpu_acquire.py gives
VALUE_BOUND = 8 * G.MEASURED_KG_ERR
# one non-uniform node set per J
NODES = {3: np.array([-1.5, 0.0, 2.0]),
         17: np.r_[-6.0, -4.0, -3.0, -2.25, -1.5, -1.0, -0.5, -0.125, 0.0, 0.25, 0.75, 1.25, 2.0, 2.5, 3.5, 4.5, 7.0],
         32: np.r_[np.linspace(-5.5, -0.5, 15) ** 3 / 30.25, 0.0, np.linspace(0.3, 5.1, 16)]}
ALL = ('kg', 'kg_hi', 'idx', 'val', 'm', 's')


def _synthetic(D, S, M, dtype):
    """tests/test_gpu_sample_argmax.py's construction: an engine with parameters set and a synthetic alpha / Li"""
    from scfgp_amd.engine import HipEngine
    seed = 0x5CF65000 + M
    K = 2 * (S + M)
    params = synth.make_params(seed + 0x0202, D, S, M, abc=(-1.0, 0.0, -1.0))
    rng = np.random.default_rng(seed)
    alpha = rng.standard_normal(K) / np.sqrt(K)
    Li = np.tril(rng.standard_normal((K, K))) / np.sqrt(K)
    eng = HipEngine(D, S, M, dtype=dtype); eng.set_params(params)
    return eng, params, alpha, Li


def _bits(a, b):
    a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _same(a, b, keys=('kg', 'kg_hi', 'm', 's')):
    return all(_bits(a[k], b[k]) for k in keys)


def _device_lines(eng, Xc, Xr, alpha, Li, noise, minimize):
    """(d, B) of the restatement from the device's own predict_cov, predict and sigma"""
    cov = eng.predict_cov(Xc, Li, Xb=Xr)
    mu_r = eng.predict(Xr, alpha, Li)[0].ravel()
    sd = eng.predict(Xc, alpha, Li)[1] if noise else eng.acquire(Xc, alpha, Li, 'ucb', beta=0.0, noise=False, want=('acq', 'sd'))['sd']
    return G.offsets(mu_r, minimize), G.slopes(cov, sd)


# ---- 1, 2. the node table bit for bit; the values at the device's own table
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('D,S,M,T,Rn', SHAPES)
def test_node_table_bit_for_bit_and_values(D, S, M, T, Rn, dtype):
    eng, params, alpha, Li = _synthetic(D, S, M, dtype)
    Xc, Xr = synth.make_X(101, T, D), synth.make_X(202, Rn, D)
    worst = 0.0
    for noise in (True, False):
        for minimize in (False, True):
            d, B = _device_lines(eng, Xc, Xr, alpha, Li, noise, minimize)
            for J, z in NODES.items():
                r = eng.acquire_kg(Xc, alpha, Li, Xr=Xr, z=z, noise=noise, minimize=minimize, want=ALL)
                m, s, lo, hi = G.node_table(d, B, z)
                assert r['m'].shape == (T, J) and _bits(r['m'], m), (noise, minimize, J)
                assert _bits(r['s'], s), (noise, minimize, J)
                assert (r['m'][:, list(z).index(0.0)] == 0.0).all()
                kg, kg_hi = G.bounds(r['m'], r['s'], lo, hi, z)
                assert (r['kg'] >= 0).all() and (r['kg'] <= r['kg_hi'] + VALUE_BOUND * kg_hi.max()).all()
                e = max(np.abs(r['kg'] - kg).max(), np.abs(r['kg_hi'] - kg_hi).max()) / kg_hi.max()
                worst = max(worst, float(e))
    print('values %s %s: max |delta| / max kg_hi = %.2e (bound %.1e)' % ((D, S, M, T, Rn), dtype, worst, VALUE_BOUND))
    assert worst <= VALUE_BOUND, worst
    eng.close()


# ---- 3. the bracket around the independent truth
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('D,S,M,T,Rn', SHAPES)
def test_bracket_against_the_exact_value_of_numpy_features(D, S, M, T, Rn, dtype):
    eng, params, alpha, Li = _synthetic(D, S, M, dtype)
    Xc, Xr = synth.make_X(101, 40, D), synth.make_X(202, Rn, D)
    kap = PC.kappa(params)
    Cc, Cr = PC.factor(Xc, Li, params, S, M), PC.factor(Xr, Li, params, S, M)
    mu_ref = O.feature_map(Xr, params, D, S, M) @ alpha
    for noise in (True, False):
        v = np.sum(Cc ** 2, axis=1)
        sd = np.sqrt(kap * (v + 1.0)) if noise else np.sqrt(kap * v)
        d_ref, B_ref = G.offsets(mu_ref), G.slopes(kap * (Cc @ Cr.T), sd)
        exact = G.kg_exact_rows(d_ref, B_ref)
        d_dev, B_dev = _device_lines(eng, Xc, Xr, alpha, Li, noise, False)
        # KG is Lipschitz in the lines: |max_r (d_r + b_r Z) - max_r (d'_r + b'_r Z)| <= max |d - d'| + max_r |b_r - b'_r| |Z|, E|Z| < 0.8;
        # d = u - max u moves by at most twice what u moves
        du = np.abs(eng.predict(Xr, alpha, Li)[0].ravel() - mu_ref).max()
        slack = 2 * du + 0.8 * np.abs(B_dev - B_ref).max(axis=1) + 1e-15 * exact.max()
        r = eng.acquire_kg(Xc, alpha, Li, Xr=Xr, noise=noise, want=('kg', 'kg_hi'))
        print('bracket %s %s noise=%d: max slack / max exact %.2e, (exact - kg) / max %.2e, (kg_hi - exact) / max %.2e'
              % ((D, S, M, Rn), dtype, noise, slack.max() / exact.max(), (exact - r['kg']).max() / exact.max(),
                 (r['kg_hi'] - exact).max() / exact.max()))
        assert (r['kg'] - slack <= exact).all() and (exact <= r['kg_hi'] + slack).all()
    eng.close()


# ---- 4. bit-level guarantees
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_rows_do_not_depend_on_position_or_chunk(dtype):
    D, S, M, T, Rn = 3, 1, 20, 32768 + 500, 33
    eng, params, alpha, Li = _synthetic(D, S, M, dtype)
    Xc, Xr = synth.make_X(101, T, D), synth.make_X(202, Rn, D)
    a = eng.acquire_kg(Xc, alpha, Li, Xr=Xr, want=ALL)
    assert a['idx'] == G.argmax(a['kg']) and _bits(a['val'], a['kg'][a['idx']])
    rows = np.r_[0:3, 126:131, 32765:32771, T - 3:T]
    b = eng.acquire_kg(Xc[rows], alpha, Li, Xr=Xr, want=ALL)
    assert _same({k: a[k][rows] for k in ('kg', 'kg_hi', 'm', 's')}, b)
    c = eng.acquire_kg(Xc, alpha, Li, Xr=Xr, want=ALL)                                     # a repeat call
    assert _same(a, c) and a['idx'] == c['idx'] and _bits(a['val'], c['val'])
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_reference_rows_are_a_set(dtype):
    D, S, M, T, Rn = SHAPES[0]
    eng, params, alpha, Li = _synthetic(D, S, M, dtype)
    Xc, Xr = synth.make_X(101, T, D), synth.make_X(202, Rn, D)
    a = eng.acquire_kg(Xc, alpha, Li, Xr=Xr, want=ALL)
    perm = np.random.default_rng(3).permutation(Rn)
    assert _same(a, eng.acquire_kg(Xc, alpha, Li, Xr=Xr[perm], want=ALL))
    assert _same(a, eng.acquire_kg(Xc, alpha, Li, Xr=np.concatenate([Xr, Xr]), want=ALL))       # R = 157 -> 314
    s1 = eng.acquire_kg(Xc, alpha, Li, want=ALL)                                                # Xr = NULL
    s2 = eng.acquire_kg(Xc, alpha, Li, Xr=Xc, want=ALL)
    assert _same(s1, s2) and s1['idx'] == s2['idx'] and _bits(s1['val'], s2['val'])
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_column_split_does_not_change_a_bit(dtype):
    D, S, M = 3, 1, 20
    eng, params, alpha, Li = _synthetic(D, S, M, dtype)
    Xc, Xr = synth.make_X(101, 700, D), synth.make_X(202, 3000, D)
    a = eng.acquire_kg(Xc, alpha, Li, Xr=Xr, want=ALL)                                         # 6 strips
    b = eng.acquire_kg(Xc[340:345], alpha, Li, Xr=Xr, want=ALL)                                # 1 strip: the columns are split further
    assert _same({k: a[k][340:345] for k in ('kg', 'kg_hi', 'm', 's')}, b)
    d, B = _device_lines(eng, Xc[340:345], Xr, alpha, Li, True, False)
    m, s, lo, hi = G.node_table(d, B, G.DEFAULT_NODES)
    assert _bits(b['m'], m) and _bits(b['s'], s)
    eng.close()


def test_f16x3_context_equals_fp32_context():
    from scfgp_amd.engine import HipEngine
    D, S, M, T, Rn = SHAPES[2]
    e32, params, alpha, Li = _synthetic(D, S, M, 'f32')
    e16 = HipEngine(D, S, M, dtype='f16x3'); e16.set_params(params)
    Xc, Xr = synth.make_X(101, T, D), synth.make_X(202, Rn, D)
    a = e32.acquire_kg(Xc, alpha, Li, Xr=Xr, want=ALL)
    b = e16.acquire_kg(Xc, alpha, Li, Xr=Xr, want=ALL)
    assert _same(a, b) and a['idx'] == b['idx'] and _bits(a['val'], b['val'])
    e32.close(); e16.close()


# ---- 5. one reference row
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_one_reference_row_gives_zero(dtype):
    D, S, M, T, Rn = SHAPES[1]
    eng, params, alpha, Li = _synthetic(D, S, M, dtype)
    Xc, Xr = synth.make_X(101, T, D), synth.make_X(202, 1, D)
    for noise in (True, False):
        r = eng.acquire_kg(Xc, alpha, Li, Xr=Xr, noise=noise, want=ALL)
        assert (r['kg'] == 0).all() and (r['kg_hi'] == 0).all() and r['idx'] == 0 and r['val'] == 0.0
    eng.close()


# ---- 6. argmax
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_argmax(dtype):
    D, S, M, T, Rn = SHAPES[0]
    eng, params, alpha, Li = _synthetic(D, S, M, dtype)
    Xc, Xr = synth.make_X(101, T, D), synth.make_X(202, Rn, D)
    r = eng.acquire_kg(Xc, alpha, Li, Xr=Xr)
    kg, idx = r['kg'], r['idx']
    assert idx == G.argmax(kg) and _bits(r['val'], kg[idx])
    r1 = eng.acquire_kg(Xc, alpha, Li, Xr=Xr, want=('idx', 'val'))                          # kg = NULL
    assert r1['idx'] == idx and _bits(r1['val'], r['val'])
    w = np.full(T, 2.0); w[idx] = 0.0; w[256:300] = 0.0
    rm = eng.acquire_kg(Xc, alpha, Li, Xr=Xr, w=w)
    assert rm['idx'] == G.argmax(kg, w) and rm['idx'] != idx and _bits(rm['val'], kg[rm['idx']]) and _bits(rm['kg'], kg)
    w1 = np.zeros(T); w1[T - 7] = 1e-300                                                   # a single eligible row
    r2 = eng.acquire_kg(Xc, alpha, Li, Xr=Xr, w=w1, want=('idx', 'val'))
    assert r2['idx'] == T - 7 and _bits(r2['val'], kg[T - 7])
    Xt = Xc.copy()                                                                         # a planted tie: a duplicated candidate row
    if idx > 0:
        Xt[0] = Xc[idx]
    else:
        Xt[T - 1] = Xc[0]
    r3 = eng.acquire_kg(Xt, alpha, Li, Xr=Xr)
    assert _bits(r3['kg'][T - 1 if idx == 0 else idx], r3['kg'][0]) and r3['idx'] == 0 and _bits(r3['val'], r['val'])
    r4 = eng.acquire_kg(np.concatenate([Xc, Xc]), alpha, Li, Xr=Xr, want=('idx', 'val'))   # the pool appended to itself
    assert r4['idx'] == idx and _bits(r4['val'], r['val'])
    eng.close()


# ---- 7. errors
_dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _raw_call(eng, Xc, Xr, alpha, Li, T=None, Rn=None, w=None, z=G.DEFAULT_NODES, J=None, mode=0, noise=1, outs='khivms', null=()):
    """scfgp_acquire_kg through ctypes with sentinel-filled outputs: (rc, outputs untouched?)"""
    T = Xc.shape[0] if T is None else T
    Rn = (0 if Xr is None else Xr.shape[0]) if Rn is None else Rn
    z = np.ascontiguousarray(z, np.float64)
    J = z.size if J is None else J
    n = max(Xc.shape[0], 1)
    bufs = {'k': np.full(n, 7.25), 'h': np.full(n, 7.25), 'v': np.full(1, 7.25), 'm': np.full((n, 32), 7.25), 's': np.full((n, 32), 7.25)}
    idx = np.full(1, -77, np.int64)
    get = lambda k: _dp(bufs[k]) if k in outs else None
    rc = eng.lib.scfgp_acquire_kg(eng.ctx, None if 'Xc' in null else _dp(Xc), T, _dp(w), _dp(Xr), Rn, None if 'alpha' in null else _dp(alpha),
                                  None if 'Li' in null else _dp(Li), None if 'z' in null else _dp(z), J, mode, noise, 0, get('k'), get('h'),
                                  idx.ctypes.data_as(C.POINTER(C.c_int64)) if 'i' in outs else None, get('v'), get('m'), get('s'))
    untouched = idx[0] == -77 and all((b == 7.25).all() for b in bufs.values())
    return rc, untouched


def test_errors_leave_the_outputs_untouched():
    from scfgp_amd.engine import HipEngine
    D, S, M, T, Rn = SHAPES[0]
    eng, params, alpha, Li = _synthetic(D, S, M, 'f64')
    Xc, Xr = synth.make_X(101, T, D), synth.make_X(202, Rn, D)
    Li = np.ascontiguousarray(Li)
    z = G.DEFAULT_NODES
    call = lambda **kw: _raw_call(eng, kw.pop('Xc', Xc), kw.pop('Xr', Xr), alpha, Li, **kw)
    assert call() == (0, False)                                   # the sentinel scheme sees a successful call
    big = np.zeros((32769, D))
    EARG = [dict(null=('Xc',)), dict(null=('alpha',)), dict(null=('Li',)), dict(null=('z',)), dict(T=0), dict(Rn=0), dict(Rn=32769),
            dict(Xc=big, Xr=None), dict(J=2), dict(z=np.linspace(-1, 1, 33)), dict(z=np.r_[z[:5], z[4], z[5:]][:31]), dict(z=z[::-1].copy()),
            dict(z=z + 0.01), dict(z=np.r_[-1.0, -0.0, 0.0, 1.0]), dict(mode=2), dict(mode=-1), dict(mode=1),
            dict(w=np.r_[np.ones(T - 1), -1.0]), dict(w=np.zeros(T)), dict(outs=''), dict(outs='v'), dict(outs='khvms')]
    for kw in EARG:
        rc, untouched = call(**dict(kw))
        assert rc == -1 and untouched, kw
        assert eng.last_error().startswith('acquire_kg:'), kw
    fresh = HipEngine(D, S, M, dtype='f64')                       # parameters not set
    assert _raw_call(fresh, Xc, Xr, alpha, Li) == (-1, True)
    fresh.close()
    NONFINITE = [dict(z=np.r_[z[:-1], np.inf]), dict(z=np.r_[np.nan, z[1:]]), dict(w=np.r_[np.ones(T - 1), np.nan]),
                 dict(w=np.r_[np.ones(T - 1), np.inf])]
    for kw in NONFINITE:
        assert call(**dict(kw)) == (-4, True), kw
    Xrbad = Xr.copy(); Xrbad[Rn - 2, 0] = np.nan                  # a non-finite u_r, found on the device
    assert call(Xr=Xrbad) == (-4, True)
    Xbad = Xc.copy(); Xbad[T - 5, 1] = np.nan                     # an eligible candidate, found on the device
    assert call(Xc=Xbad) == (-4, True)
    w = np.ones(T); w[T - 5] = 0.0
    assert call(Xc=Xbad, w=w) == (0, False)                       # not eligible: not an error
    good = eng.acquire_kg(Xc, alpha, Li, Xr=Xr, w=w)
    r = eng.acquire_kg(Xbad, alpha, Li, Xr=Xr, w=w)
    assert r['idx'] == good['idx'] and _bits(np.delete(r['kg'], T - 5), np.delete(good['kg'], T - 5))
    with pytest.raises(FloatingPointError):
        eng.acquire_kg(Xbad, alpha, Li, Xr=Xr)
    zero = np.zeros_like(Li)                                      # v = 0: the latent sigma is 0, the predictive one is not
    with pytest.raises(FloatingPointError):
        eng.acquire_kg(Xc, alpha, zero, Xr=Xr, noise=False)
    r0 = eng.acquire_kg(Xc, alpha, zero, Xr=Xr, noise=True, want=('kg', 'kg_hi'))
    assert (r0['kg'] == 0).all() and (r0['kg_hi'] == 0).all()
    with pytest.raises(ValueError):
        eng.acquire_kg(Xc, alpha, Li, Xr=Xr, mode='raw')          # no X scaler registered
    with pytest.raises(ValueError):
        eng.acquire_kg(Xc, alpha, Li, Xr=Xr, want=('bogus',))
    eng.close()


# ---- 8. the training state
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_training_state_survives(dtype):
    from scfgp_amd.engine import HipEngine
    D, S, M, N = 20, 20, 280, 1500
    params = synth.make_params(7, D, S, M, abc=(-1.0, 0.0, -1.0))
    X = synth.make_X(7, N, D)
    y = np.sin(3 * X[:, :1]) + 0.1 * synth.normal(10, 0, N)[:, None]
    eng = HipEngine(D, S, M, dtype=dtype); eng.set_params(params); eng.set_data(X, y)
    c0, g0, a0, L0 = eng.eval(want_grad=True)
    c0, g0, a0, L0 = float(c0), g0.copy(), a0.copy(), L0.copy()
    r = eng.acquire_kg(synth.make_X(9, 1300, D), a0, L0, Xr=synth.make_X(11, 900, D), want=ALL)
    assert np.isfinite(r['kg_hi']).all() and (r['kg'] >= 0).all()
    c1, g1, a1, L1 = eng.eval(want_grad=True)
    assert float(c1) == c0 and np.array_equal(g1, g0) and np.array_equal(a1, a0) and np.array_equal(L1, L0)
    eng.close()


# ---- 9. facade
def test_facade():
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
    pool = np.column_stack([rng.uniform(-2, 2, (500, 2)), np.full(500, 4.0), rng.uniform(-2, 2, 500)])
    ref = np.column_stack([rng.uniform(-2, 2, (700, 2)), np.full(700, 4.0), rng.uniform(-2, 2, 700)])
    eng = model.pred_func.__self__.engine
    fp, fr = (np.ascontiguousarray(model.X_scaler.forward_transform(x), dtype=np.float64) for x in (pool, ref))
    def rel(a, b):                                                      # an all-zero kg (no second winner within the nodes) must agree exactly
        nb = np.linalg.norm(b)
        return float(np.linalg.norm(a - b) / nb) if nb > 0 else float(np.abs(a).max())
    wide = np.r_[-60.0, -30.0, -15.0, np.linspace(-8.0, 8.0, 25), 15.0, 30.0, 60.0]
    for minimize, noise, nodes in ((False, True, None), (True, True, None), (False, False, None), (False, False, wide)):
        r = model.kg(pool, ref, nodes=nodes, noise=noise, minimize=minimize)
        e = eng.acquire_kg(fp, model.alpha, model.Li, Xr=fr, z=nodes, noise=noise, minimize=minimize, want=('kg', 'kg_hi', 'idx', 'val'))
        assert set(r) == {'kg', 'kg_hi', 'idx', 'val'} and r['kg'].shape == (500,)
        print('facade minimize=%d noise=%d: max kg %.2e max kg_hi %.2e; raw against scaled: kg %.2e kg_hi %.2e'
              % (minimize, noise, r['kg'].max(), r['kg_hi'].max(), rel(r['kg'], e['kg']), rel(r['kg_hi'], e['kg_hi'])))
        assert r['kg_hi'].max() > 0
        assert rel(r['kg'], e['kg']) < 1e-12 and rel(r['kg_hi'], e['kg_hi']) < 1e-12
        assert r['idx'] == G.argmax(r['kg']) and (r['kg'] <= r['kg_hi'] + 1e-12 * r['kg_hi'].max()).all()
    s = model.kg(pool)                                                  # the pool is its own reference set
    assert _bits(s['kg'], model.kg(pool, pool)['kg'])
    w = np.ones(500); w[s['idx']] = 0.0
    assert model.kg(pool, weights=w)['idx'] == G.argmax(s['kg'], w)
    other = SCFGP(sparsity=3, nfeats=12)
    other.pred_func = lambda Xs, alpha, Li: None
    with pytest.raises(TypeError):
        other.kg(pool)
