"""GPU tier of scfgp_acquire (acquire.hip): mu / sd against predict bit for bit; every kind against the numpy restatement
(tests/acquire_ref.py) evaluated at the call's own mu, sd; the argmax rule, ties, masks and the chunk boundary; position independence;
the gradient against finite differences of the entry point's own values and against the restatement's partials chained with
predict_grad; the f16x3 context; every error with untouched outputs; the survival of the training state; the SCFGP facade."""
import ctypes as C

import numpy as np
import pytest

from scfgp_amd import synth
from scfgp_amd.scaler import Scaler
from tests import acquire_ref as A
from tests import sample_ref as R

pytestmark = pytest.mark.gpu

# A: K = 42, ragged everything; B: a second, ragged chunk
SHAPE_A = (3, 1, 20, 700)
SHAPE_B = (5, 4, 60, 32768 + 500)
# The device against the restatement at the same mu, sd: only the fp64 acquisition arithmetic is under test, in every context.  8 x the
# restatement's own measured error (the device's erfcx / erfc / log / exp are other implementations at a few ulp each; MES sums up to
# 1024 non-negative terms).  Measured on the device (worst over shapes, dtypes, noise, directions, incumbents):
#     ucb 0, pi 5.7e-14, ei 3.4e-13, logei 9.8e-16, mes 1.5e-15
PARITY_BOUND = {k: 8 * v for k, v in A.MEASURED_KIND_ERR.items()}
# norm-wise, against the restatement's partials chained with predict_grad's dmu, dstd: 8 x the value first measured on the device, 1.7e-16
# (both dtypes: the gradient kernels are predict_grad's own, so only the fp64 combine differs)
CHAIN_BOUND = 8 * 1.7e-16


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


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def _incumbents(mu, sd, minimize):
    """best in {median u, max u, max u + 5 median sigma, max u + 30 median sigma}, back in mu's direction"""
    sgn = -1.0 if minimize else 1.0
    u, ms = sgn * mu, float(np.median(sd))
    return [sgn * b for b in (float(np.median(u)), float(u.max()), float(u.max()) + 5 * ms, float(u.max()) + 30 * ms)]


# ---- 1. mu, sd against predict
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('D,S,M,T', [SHAPE_A, SHAPE_B, (5, 4, 60, 70001)])
def test_mu_sd_against_predict(D, S, M, T, dtype):
    eng, params, alpha, Li = _synthetic(D, S, M, dtype)
    Xs = synth.make_X(101, T, D)
    mu_p, sd_p = eng.predict(Xs, alpha, Li)
    r1 = eng.acquire(Xs, alpha, Li, 'ucb', beta=1.0, noise=True, want=('acq', 'mu', 'sd'))
    assert r1['mu'].shape == (T,) and _bits(r1['mu'], mu_p.ravel()) and _bits(r1['sd'], sd_p)
    r0 = eng.acquire(Xs, alpha, Li, 'ucb', beta=1.0, noise=False, want=('acq', 'mu', 'sd'))
    assert _bits(r0['mu'], mu_p.ravel())
    kap = R.kappa(params)
    v = r0['sd'] ** 2 / kap
    cmp = np.sqrt(sd_p ** 2 - kap)                              # the comparison quantity cancels: 4 eps (1 + v) / v is ITS bound
    err = np.abs(r0['sd'] - cmp) / cmp
    assert (err <= 4 * np.finfo(float).eps * (1 + v) / v).all(), float((err * v / (1 + v)).max())
    eng.close()


# ---- 2. elementwise parity
def _rows_for_mes(T):
    return np.unique(np.r_[0:300, 32700:32900, T - 200:T] % T)


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('D,S,M,T', [SHAPE_A, SHAPE_B])
def test_elementwise_parity(D, S, M, T, dtype):
    eng, params, alpha, Li = _synthetic(D, S, M, dtype)
    Xs = synth.make_X(101, T, D)
    worst = dict.fromkeys(A.KINDS, 0.0)
    sel = _rows_for_mes(T)
    for noise in (False, True):
        for minimize in (False, True):
            kw = dict(noise=noise, minimize=minimize, want=('acq', 'mu', 'sd'))
            r = eng.acquire(Xs, alpha, Li, 'ucb', beta=2.5, **kw)
            mu, sd = r['mu'], r['sd']
            ref, _, _ = A.acquire('ucb', mu, sd, beta=2.5, minimize=minimize)
            worst['ucb'] = max(worst['ucb'], A.kind_error('ucb', r['acq'], ref, mu, sd, 2.5))
            for best in _incumbents(mu, sd, minimize):
                for kind in ('pi', 'ei', 'logei'):
                    r = eng.acquire(Xs, alpha, Li, kind, best=best, xi=0.01, **kw)
                    assert _bits(r['mu'], mu) and _bits(r['sd'], sd)
                    ref, _, _ = A.acquire(kind, mu, sd, best=best, xi=0.01, minimize=minimize)
                    worst[kind] = max(worst[kind], A.kind_error(kind, r['acq'], ref))
            ms = float(np.median(sd))
            sgn = -1.0 if minimize else 1.0
            for ns in (1, 7, 64, 300, 1024):
                _, fs = eng.sample_argmax(Xs, alpha, Li, ns, seed=9, minimize=minimize)
                for off in (0.0, -2.0, 30.0):                   # the offsets make g take both signs and reach the tail
                    f = fs + sgn * off * ms
                    r = eng.acquire(Xs, alpha, Li, 'mes', fstar=f, **kw)
                    assert (r['acq'] >= 0).all()
                    ref, _, _ = A.acquire('mes', mu[sel], sd[sel], fstar=f, minimize=minimize)
                    worst['mes'] = max(worst['mes'], A.kind_error('mes', r['acq'][sel], ref))
    print('parity %s %s: %s' % ((D, S, M, T), dtype, ' '.join('%s=%.2e' % kv for kv in worst.items())))
    for kind in A.KINDS:
        assert worst[kind] <= PARITY_BOUND[kind], (kind, worst[kind], PARITY_BOUND[kind])
    eng.close()


# ---- 3. argmax
def _kind_args(eng, Xs, alpha, Li, kind):
    if kind == 'mes':
        return dict(fstar=eng.sample_argmax(Xs[:2000], alpha, Li, 7, seed=3)[1])
    mu = eng.acquire(Xs[:2000], alpha, Li, 'ucb', beta=0.0, want=('acq',))['acq']
    return dict(best=float(np.median(mu)), xi=0.0)


@pytest.mark.parametrize('kind', ['ei', 'mes'])
@pytest.mark.parametrize('dtype,shape', [('f64', SHAPE_A), ('f32', SHAPE_B)])
def test_argmax(dtype, shape, kind):
    D, S, M, T = shape
    eng, params, alpha, Li = _synthetic(D, S, M, dtype)
    Xs = synth.make_X(101, T, D)
    kw = _kind_args(eng, Xs, alpha, Li, kind)
    r = eng.acquire(Xs, alpha, Li, kind, **kw)
    acq, idx = r['acq'], r['idx']
    assert idx == A.argmax(acq) and _bits(r['val'], acq[idx])
    r1 = eng.acquire(Xs, alpha, Li, kind, want=('argmax',), **kw)                       # acq = NULL
    assert r1['idx'] == idx and _bits(r1['val'], r['val'])
    r2 = eng.acquire(np.concatenate([Xs, Xs]), alpha, Li, kind, want=('argmax',), **kw)   # every value ties with its copy
    assert r2['idx'] == idx and _bits(r2['val'], r['val'])
    r3 = eng.acquire(np.repeat(Xs, 2, axis=0), alpha, Li, kind, want=('argmax',), **kw)
    assert r3['idx'] == 2 * idx and _bits(r3['val'], r['val'])
    w = np.full(T, 2.0); w[idx] = 0.0                              # the winner excluded
    blk = 256 * ((idx // 256 + 1) % (T // 256))
    w[blk:blk + 256] = 0.0                                         # a whole workgroup's rows
    rm = eng.acquire(Xs, alpha, Li, kind, w=w, **kw)
    assert rm['idx'] == A.argmax(acq, w) and rm['idx'] != idx and _bits(rm['val'], acq[rm['idx']]) and _bits(rm['acq'], acq)
    w1 = np.zeros(T); w1[T - 123] = 1e-300                         # a single eligible row
    r4 = eng.acquire(Xs, alpha, Li, kind, w=w1, want=('argmax',), **kw)
    assert r4['idx'] == T - 123 and _bits(r4['val'], acq[T - 123])
    for wt in (np.ones(T), 3.5e7 * np.ones(T)):                    # positive values are not multiplied in
        r5 = eng.acquire(Xs, alpha, Li, kind, w=wt, want=('argmax',), **kw)
        assert r5['idx'] == idx and _bits(r5['val'], r['val'])
    eng.close()


# ---- 4. position independence
@pytest.mark.parametrize('kind', ['logei', 'mes'])
def test_position_independence(kind):
    D, S, M, T = SHAPE_B
    eng, params, alpha, Li = _synthetic(D, S, M, 'f32')
    Xs = synth.make_X(101, T, D)
    kw = _kind_args(eng, Xs, alpha, Li, kind)
    want = ('acq', 'mu', 'sd', 'grad')
    a = eng.acquire(Xs, alpha, Li, kind, want=want, **kw)
    b = eng.acquire(np.concatenate([Xs[70:], Xs[:70]]), alpha, Li, kind, want=want, **kw)
    for k in want:
        assert _bits(np.concatenate([a[k][70:], a[k][:70]]), b[k]), k
    eng.close()


# ---- 5. gradient
def _all_kind_args(eng, Xs, alpha, Li, noise, minimize):
    r = eng.acquire(Xs, alpha, Li, 'ucb', beta=0.0, minimize=minimize, noise=noise, want=('acq', 'mu', 'sd'))
    best = (-1.0 if minimize else 1.0) * float(np.median(r['acq']))
    fs = eng.sample_argmax(Xs, alpha, Li, 7, seed=3, minimize=minimize)[1]
    return {'ucb': dict(beta=1.5), 'pi': dict(best=best, xi=0.01), 'ei': dict(best=best, xi=0.01), 'logei': dict(best=best, xi=0.01),
            'mes': dict(fstar=fs)}


def _fd(f, X, cols, h=1e-6):
    """central differences of f (rows -> values (T,)) in the listed columns, all rows in one call (tests/test_gpu_predict_grad.py)"""
    T, Dr = X.shape
    batch = [X]
    for c in cols:
        for s in (1, -1):
            Xp = X.copy(); Xp[:, c] += s * h * max(1.0, abs(X[:, c]).max()); batch.append(Xp)
    v = np.asarray(f(np.vstack(batch))).reshape(-1)
    g = np.zeros((T, Dr))
    for k, c in enumerate(cols):
        hh = 2 * h * max(1.0, abs(X[:, c]).max())
        g[:, c] = (v[(1 + 2 * k) * T:(2 + 2 * k) * T] - v[(2 + 2 * k) * T:(3 + 2 * k) * T]) / hh
    return g


@pytest.mark.parametrize('D,S,M,T', [SHAPE_A, SHAPE_B])
def test_gradient_scaled_mode_against_finite_differences(D, S, M, T):
    eng, params, alpha, Li = _synthetic(D, S, M, 'f64')
    Xs = synth.make_X(101, T, D)
    sel = np.unique(np.r_[0:60, 32740:32800, T - 60:T] % T)
    for noise, minimize in ((False, False), (True, True)):
        for kind, kw in _all_kind_args(eng, Xs, alpha, Li, noise, minimize).items():
            kw = dict(kw, noise=noise, minimize=minimize)
            r = eng.acquire(Xs, alpha, Li, kind, want=('acq', 'grad'), **kw)
            assert r['grad'].shape == (T, D)
            assert _bits(eng.acquire(Xs, alpha, Li, kind, want=('acq',), **kw)['acq'], r['acq'])      # grad = NULL: the same acq
            fd = _fd(lambda X: eng.acquire(X, alpha, Li, kind, want=('acq',), **kw)['acq'], Xs[sel], range(D))
            e = rel(r['grad'][sel], fd)
            print('fd %s noise=%d minimize=%d: %.2e' % (kind, noise, minimize, e))
            assert e < 1e-5, (kind, e)
    eng.close()


def _scaled_problem(xalgo, yalgo, seed=5, N=600, T=50):
    """tests/test_gpu_predict_grad.py's problem: an engine trained on scaled data of 4 raw columns, one of them constant"""
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
def test_gradient_raw_mode_through_every_x_scaler(xalgo):
    eng, xs, ys, alpha, Li, Xr = _scaled_problem(xalgo, 'normal')
    cols = xs.data['cols']
    Xs = np.ascontiguousarray(xs.forward_transform(Xr))
    for kind, kw in _all_kind_args(eng, Xs, alpha, Li, True, False).items():
        kw = dict(kw, noise=True)
        r = eng.acquire(Xr, alpha, Li, kind, mode='raw', want=('acq', 'grad'), **kw)
        assert r['grad'].shape == (Xr.shape[0], 4) and np.all(r['grad'][:, 2] == 0)
        fd = _fd(lambda X: eng.acquire(X, alpha, Li, kind, mode='raw', want=('acq',), **kw)['acq'], Xr, cols)
        e = rel(r['grad'], fd)
        print('fd raw %s %s: %.2e' % (xalgo, kind, e))
        assert e < 1e-5, (kind, e)
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('D,S,M,T', [SHAPE_A, SHAPE_B])
def test_gradient_against_chained_partials(D, S, M, T, dtype):
    eng, params, alpha, Li = _synthetic(D, S, M, dtype)
    Xs = synth.make_X(101, T, D)
    _, sd_star, dmu, dstd = eng.predict_grad(Xs, alpha, Li)
    worst = 0.0
    for noise, minimize in ((False, False), (True, False), (False, True)):
        for kind, kw in _all_kind_args(eng, Xs, alpha, Li, noise, minimize).items():
            r = eng.acquire(Xs, alpha, Li, kind, noise=noise, minimize=minimize, want=('acq', 'mu', 'sd', 'grad'), **kw)
            _, au, as_ = A.acquire(kind, r['mu'], r['sd'], minimize=minimize, **kw)
            dsig = dstd if noise else dstd * (sd_star / r['sd'])[:, None]
            ref = (-1.0 if minimize else 1.0) * au[:, None] * dmu + as_[:, None] * dsig
            worst = max(worst, rel(r['grad'], ref))
    print('chain %s %s: %.2e' % ((D, S, M, T), dtype, worst))
    assert worst <= CHAIN_BOUND
    eng.close()


# ---- 6. f16x3
def test_f16x3_context_equals_fp32_context():
    from scfgp_amd.engine import HipEngine
    D, S, M, T = 64, 32, 1024, 33000
    e32, params, alpha, Li = _synthetic(D, S, M, 'f32')
    e16 = HipEngine(D, S, M, dtype='f16x3'); e16.set_params(params)
    Xs = synth.make_X(202, T, D)
    fs = e32.sample_argmax(Xs[:3000], alpha, Li, 16, seed=1)[1]
    want = ('acq', 'argmax', 'mu', 'sd', 'grad')
    for kind, kw in (('ei', dict(best=0.1, xi=0.0)), ('mes', dict(fstar=fs))):
        a = e32.acquire(Xs, alpha, Li, kind, want=want, **kw)
        b = e16.acquire(Xs, alpha, Li, kind, want=want, **kw)
        assert a['idx'] == b['idx'] and _bits(a['val'], b['val'])
        for k in ('acq', 'mu', 'sd', 'grad'):
            assert _bits(a[k], b[k]), k
    e32.close(); e16.close()


# ---- 7. errors and state
_dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _raw_call(eng, Xs, alpha, Li, T=None, w=None, kind=2, par=(0.0, 0.0), npar=None, fstar=None, nstar=None, mode=0, outs='aivmsg',
              null=()):
    """scfgp_acquire through ctypes with sentinel-filled outputs: (rc, outputs untouched?)"""
    T = Xs.shape[0] if T is None else T
    n = max(Xs.shape[0], 1)
    par = None if par is None else np.array(par, np.float64)
    bufs = {'a': np.full(n, 7.25), 'v': np.full(1, 7.25), 'm': np.full(n, 7.25), 's': np.full(n, 7.25), 'g': np.full((n, eng.D), 7.25)}
    idx = np.full(1, -77, np.int64)
    get = lambda k: _dp(bufs[k]) if k in outs else None
    rc = eng.lib.scfgp_acquire(eng.ctx, None if 'Xs' in null else _dp(Xs), T, _dp(w), None if 'alpha' in null else _dp(alpha),
                               None if 'Li' in null else _dp(Li), kind, _dp(par), (0 if par is None else par.size) if npar is None else npar,
                               _dp(fstar), (0 if fstar is None else fstar.size) if nstar is None else nstar, mode, 0, 0, get('a'),
                               idx.ctypes.data_as(C.POINTER(C.c_int64)) if 'i' in outs else None, get('v'), get('m'), get('s'), get('g'))
    untouched = idx[0] == -77 and all((b == 7.25).all() for b in bufs.values())
    return rc, untouched


def test_errors_leave_the_outputs_untouched():
    from scfgp_amd.engine import HipEngine
    D, S, M, T = SHAPE_A
    eng, params, alpha, Li = _synthetic(D, S, M, 'f64')
    Xs = synth.make_X(101, T, D)
    Li = np.ascontiguousarray(Li)
    f3 = np.array([0.1, 0.2, 0.3])
    call = lambda **kw: _raw_call(eng, Xs, alpha, Li, **kw)
    assert call() == (0, False)                                   # the sentinel scheme sees a successful call
    EARG = [dict(null=('Xs',)), dict(null=('alpha',)), dict(null=('Li',)), dict(T=0), dict(kind=-1), dict(kind=5), dict(mode=2), dict(mode=-1),
            dict(npar=1), dict(kind=0, par=(1.0, 0.0)), dict(kind=4, par=None, npar=1, fstar=f3), dict(par=None, npar=2),
            dict(kind=0, par=(-0.5,)), dict(par=(0.0, -1e-3)), dict(kind=4, par=None), dict(kind=4, par=None, fstar=f3, nstar=0),
            dict(kind=4, par=None, fstar=np.zeros(1025)), dict(fstar=f3), dict(mode=1),
            dict(w=np.r_[np.ones(T - 1), -1.0]), dict(w=np.zeros(T)), dict(outs='ms'), dict(outs='avms')]
    for kw in EARG:
        rc, untouched = call(**kw)
        assert rc == -1 and untouched, kw
        assert eng.last_error().startswith('acquire:'), kw
    fresh = HipEngine(D, S, M, dtype='f64')                       # parameters not set
    assert _raw_call(fresh, Xs, alpha, Li) == (-1, True)
    fresh.close()
    NONFINITE = [dict(par=(np.nan, 0.0)), dict(par=(0.0, np.inf)), dict(kind=0, par=(np.inf,)),
                 dict(kind=4, par=None, fstar=np.array([0.1, np.nan])), dict(w=np.r_[np.ones(T - 1), np.nan]), dict(w=np.r_[np.ones(T - 1), np.inf])]
    for kw in NONFINITE:
        assert call(**kw) == (-4, True), kw
    Xbad = Xs.copy(); Xbad[T - 5, 1] = np.nan                     # found on the device
    assert _raw_call(eng, Xbad, alpha, Li) == (-4, True)
    w = np.ones(T); w[T - 5] = 0.0
    assert _raw_call(eng, Xbad, alpha, Li, w=w) == (0, False)     # not eligible: not an error
    r = eng.acquire(Xbad, alpha, Li, 'ei', best=0.0, w=w)
    assert r['idx'] != T - 5 and np.isfinite(np.delete(r['acq'], T - 5)).all()
    with pytest.raises(FloatingPointError):
        eng.acquire(Xbad, alpha, Li, 'ei', best=0.0)
    zero = np.zeros_like(Li)                                      # v = 0: the latent sigma is 0, the predictive one is not
    with pytest.raises(FloatingPointError):
        eng.acquire(Xs, alpha, zero, 'logei', best=0.0, noise=False)
    assert np.isfinite(eng.acquire(Xs, alpha, zero, 'logei', best=0.0, noise=True)['acq']).all()
    with pytest.raises(ValueError):
        eng.acquire(Xs, alpha, Li, 'bogus', best=0.0)
    with pytest.raises(ValueError):
        eng.acquire(Xs, alpha, Li, 'ei', best=0.0, mode='raw')      # no X scaler registered
    eng.close()


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
    Xs = synth.make_X(9, 33000, D)
    eng.acquire(Xs, a0, L0, 'ei', best=0.0, want=('acq', 'argmax', 'grad'))
    eng.acquire(Xs, a0, L0, 'mes', fstar=np.array([1.0, 1.2]))
    c1, g1, a1, L1 = eng.eval(want_grad=True)
    assert float(c1) == c0 and np.array_equal(g1, g0) and np.array_equal(a1, a0) and np.array_equal(L1, L0)
    eng.close()


# ---- 8. facade
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
    owner = model.pred_func.__self__
    mu_s, sd_s = owner.pred_raw(pool, model.X_scaler, model.alpha, model.Li)          # scaled units
    r = model.acquire(pool, 'ei', noise=True, want=('acq', 'argmax', 'mu', 'sd'))
    assert _bits(r['mu'], np.asarray(mu_s).ravel()) and _bits(r['sd'], np.asarray(sd_s).ravel())
    ref, _, _ = A.acquire('ei', r['mu'], r['sd'], best=float(model.y.max()), xi=0.0)
    assert A.kind_error('ei', r['acq'], ref) <= PARITY_BOUND['ei'] and r['idx'] == A.argmax(r['acq'])
    best_raw = float(y[:240].max())
    r2 = model.acquire(pool, 'ei', best=best_raw, noise=True)                          # the raw incumbent goes through the y scaler
    assert np.allclose(r2['acq'], r['acq'], rtol=1e-9, atol=0)
    m = model.mes(pool, 32, seed=4)
    _, fs = owner.sample_argmax_raw(pool, model.X_scaler, model.alpha, model.Li, 32, seed=4)
    m2 = model.acquire(pool, 'mes', fstar=fs)
    assert _bits(m['fstar'], fs) and _bits(m['acq'], m2['acq']) and m['idx'] == m2['idx']
    lo, hi = pool.min(0), pool.max(0)
    Xb, val, idx, conv = model.acquire_maximize(pool, 'logei', starts=6, max_iter=25)
    acq = model.acquire(pool, 'logei', want=('acq',))['acq']
    assert Xb.shape == (6, 4) and (Xb >= lo).all() and (Xb <= hi).all() and (val >= acq[idx]).all()
    assert idx.tolist() == np.argsort(-acq, kind='stable')[:6].tolist()
    Xb2, val2, idx2, conv2 = model.acquire_maximize(pool, 'logei', starts=6, max_iter=25)
    assert _bits(Xb, Xb2) and _bits(val, val2) and np.array_equal(idx, idx2) and np.array_equal(conv, conv2)
