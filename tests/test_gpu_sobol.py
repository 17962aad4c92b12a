"""GPU tier of the closed-form Sobol indices (sobol.hip: scfgp_sobol): every output against the numpy restatement (tests/sobol_ref.py)
under the device bound of DESIGN 4.21 at the eight geometry classes and at the sizes where the pair kernel takes another path (J a
multiple of its tile edge 8 and one more; more than one run of k blocks per unit row; more than one group of inputs), the point-mass
and the exact-zero cases, the five bit-level promises of include/scfgp_hip.h, the refusals, the training state, and the SCFGP facade
(sobol, integral).  K <= 608 everywhere."""
import ctypes as C

import numpy as np
import pytest

from oracle import scfgp_oracle as O
from scfgp_amd import synth
from scfgp_amd._lib import dptr
from tests import gradcov_ref
from tests import sobol_ref as R

pytestmark = pytest.mark.gpu

ALL = ('f0', 'V', 'Vmain', 'Vtot', 'phibar')


def _engine(D, S, M, dtype, params):
    from scfgp_amd.engine import HipEngine
    eng = HipEngine(D, S, M, dtype=dtype); eng.set_params(params)
    return eng


def _check(eng, params, D, S, M, kind, p0, p1, W, tag):
    out = eng.sobol(kind, p0, p1, W, want=ALL)
    ref = R.sobol(params, D, S, M, kind, p0, p1, W)
    ratios = R.worst_ratio(out, ref, D)
    print('sobol %s %s: error / bound %s' % (tag, (D, S, M), ' '.join('%s=%.2e' % kv for kv in sorted(ratios.items()))))
    assert sorted(ratios) == sorted(ALL)
    assert all(v <= 1.0 for v in ratios.values()), ratios
    return out, ref


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('D,S,M', gradcov_ref.GEOMETRIES)
def test_parity_over_the_geometry_classes(D, S, M, dtype):
    params, W = R.parity_inputs(D, S, M)
    eng = _engine(D, S, M, dtype, params)
    out, ref = _check(eng, params, D, S, M, *R.mixed_measure(D), W, dtype)
    assert out['Vmain'].shape == (2, D) and out['Vtot'].shape == (2, D) and out['V'].shape == (2,) and out['phibar'].shape == (2 * (S + M),)
    assert np.allclose(out['f0'], out['phibar'] @ W, rtol=0, atol=float(R.bounds(ref, D)['f0'].max()) * 2)
    eng.close()


# (8, 4, 300): J = 304 = 38 tiles of 8, so a row of the triangle is cut into up to three units; (3, 2, 30) / (3, 2, 31): J = 32 and 33,
# a multiple of the tile edge and one more
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('D,S,M,nw', [(8, 4, 300, 3), (3, 2, 30, 2), (3, 2, 31, 2)])
def test_parity_at_the_tile_edges(D, S, M, nw, dtype):
    params, W = R.parity_inputs(D, S, M)
    if nw == 3:
        W = np.column_stack((W, W[:, 0] - 2.0 * W[:, 1]))
    eng = _engine(D, S, M, dtype, params)
    _check(eng, params, D, S, M, *R.mixed_measure(D), W, dtype)
    eng.close()


@pytest.mark.parametrize('D,S,M,group', [(70, 5, 60, 7), (40, 33, 20, 14), (7, 12, 3, 1)])
def test_the_group_size_changes_no_bit(D, S, M, group):
    """promise 5: ten groups instead of five at D = 70, three at D = 40, one input per group at D = 7"""
    params, W = R.parity_inputs(D, S, M)
    eng = _engine(D, S, M, 'f64', params)
    m = R.mixed_measure(D)
    a = eng.sobol(*m, W, want=ALL)
    eng.set_option('test_sobol_group', group)
    b, _ = _check(eng, params, D, S, M, *m, W, 'group %d' % group)
    eng.set_option('test_sobol_group', 1000)                     # the option can only lower the group size
    c = eng.sobol(*m, W, want=ALL)
    for k in ALL:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_point_mass_measure_gives_predict_and_no_variance(dtype):
    D, S, M = 7, 12, 3
    params, W = R.parity_inputs(D, S, M)
    x = synth.make_X(11, 1, D)
    eng = _engine(D, S, M, dtype, params)
    out, ref = _check(eng, params, D, S, M, None, x[0], x[0], W, 'point mass ' + dtype)
    bd = R.bounds(ref, D)
    mu = O.predict(x, W[:, 0], np.eye(W.shape[0]), params, S, M)[0]
    assert abs(out['f0'][0] - float(mu[0, 0])) <= bd['f0'][0]
    for k in ('V', 'Vmain', 'Vtot'):
        assert np.all(np.abs(out[k]) <= bd[k]), k
    eng.close()


def test_a_factor_that_is_exactly_zero():
    """input 2 normal with sd 1e3: psi underflows to 0 for nearly every pair, and the leave-one-out products without it must not"""
    D, S, M = 7, 12, 3
    params, W = R.parity_inputs(D, S, M)
    kind, p0, p1 = R.mixed_measure(D)
    kind[2] = 1; p0[2] = 0.5; p1[2] = 1e3
    eng = _engine(D, S, M, 'f64', params)
    out, ref = _check(eng, params, D, S, M, kind, p0, p1, W, 'zero psi')
    assert all(np.all(np.isfinite(out[k])) for k in ALL)
    assert ref['Vtot'][0, 2] / ref['V'][0] > 0.99 and 0.3 < ref['Vmain'][0, 2] / ref['V'][0] < 0.9
    eng.close()


def test_promises_bit_for_bit():
    D, S, M = 1, 2, 2
    params, W2 = R.parity_inputs(D, S, M)
    rng = np.random.default_rng(3)
    W = np.column_stack((W2, rng.standard_normal((W2.shape[0], 1022))))
    m = R.mixed_measure(D)
    outs = {}
    for dtype in ('f64', 'f32', 'f16x3'):
        eng = _engine(D, S, M, dtype, params)
        full = eng.sobol(*m, W, want=ALL)
        again = eng.sobol(*m, W, want=ALL)
        for k in ALL:                                              # 1: the same bits on every run
            assert np.array_equal(full[k], again[k]), k
        for nw in (1, 5, 33):                                      # 2: fewer columns return a prefix
            part = eng.sobol(*m, W[:, :nw], want=ALL)
            for k in ('f0', 'V', 'Vmain', 'Vtot'):
                assert np.array_equal(part[k], full[k][:nw]), (k, nw)
            assert np.array_equal(part['phibar'], full['phibar'])
        alone = eng.sobol(*m, np.ascontiguousarray(W[:, 700]), want=ALL)        # ... and a column alone is that column
        for k in ('f0', 'V', 'Vmain', 'Vtot'):
            assert np.array_equal(alone[k][0], full[k][700]), k
        outs[dtype] = full
        eng.close()
    for k in ALL:                                                  # 4: the three compute modes agree
        assert np.array_equal(outs['f64'][k], outs['f32'][k]) and np.array_equal(outs['f32'][k], outs['f16x3'][k]), k


@pytest.mark.parametrize('D,S,M', [(7, 12, 3), (40, 33, 20)])
def test_an_output_does_not_depend_on_which_others_are_asked_for(D, S, M):
    """promise 3, with every subset of the optional outputs"""
    params, W = R.parity_inputs(D, S, M)
    eng = _engine(D, S, M, 'f32', params)
    m = R.mixed_measure(D)
    full = eng.sobol(*m, W, want=ALL)
    for mask in range(1, 32):
        want = tuple(k for i, k in enumerate(ALL) if mask >> i & 1)
        part = eng.sobol(*m, W, want=want)
        assert sorted(part) == sorted(want)
        for k in want:
            assert np.array_equal(part[k], full[k]), (want, k)
    only = eng.sobol(*m, None, want=('phibar',))                   # W may be missing when only phibar is asked for
    assert np.array_equal(only['phibar'], full['phibar'])
    eng.close()


def test_refusals_leave_the_outputs_alone():
    D, S, M = 7, 12, 3
    K = 2 * (S + M)
    params, W = R.parity_inputs(D, S, M)
    W = np.ascontiguousarray(W)
    eng = _engine(D, S, M, 'f64', params)
    kind, p0, p1 = R.mixed_measure(D)
    outs = [np.full(2, 7.0), np.full(2, 7.0), np.full((2, D), 7.0), np.full((2, D), 7.0), np.full(K, 7.0)]
    keep = []

    def ip(v):
        keep.append(np.ascontiguousarray(v, dtype=np.int32))
        return keep[-1].ctypes.data_as(C.POINTER(C.c_int32))

    def call(kind_=kind, p0_=p0, p1_=p1, W_=W, nw=2, outs_=outs):
        return eng.lib.scfgp_sobol(eng.ctx, None if kind_ is None else ip(kind_), dptr(p0_), dptr(p1_), dptr(W_), nw, *[dptr(o) for o in outs_])

    def changed(v, i, x):
        v = np.array(v, dtype=np.float64); v.reshape(-1)[i] = x
        return v

    k3 = kind.copy(); k3[3] = 2
    cases = [
        (dict(p0_=None), -1, 'sobol: p0 and p1 are needed'),
        (dict(p1_=None), -1, 'sobol: p0 and p1 are needed'),
        (dict(outs_=[None] * 5), -1, 'sobol: no output asked for'),
        (dict(W_=None), -1, 'sobol: W is needed for f0, V, Vmain and Vtot'),
        (dict(nw=0), -1, 'sobol: nw must lie in 1..1024'),
        (dict(nw=1025), -1, 'sobol: nw must lie in 1..1024'),
        (dict(kind_=k3), -1, 'sobol: kind[3] must be 0 (uniform) or 1 (normal)'),
        (dict(p1_=changed(p1, 4, -0.5)), -1, 'sobol: input 4: p1 < p0 on a uniform input'),
        (dict(p1_=changed(p1, 5, -0.5)), -1, 'sobol: input 5: p1 (the standard deviation) is negative'),
        (dict(p0_=changed(p0, 1, np.nan)), -4, 'sobol: non-finite measure at input 1'),
        (dict(p1_=changed(p1, 6, np.inf)), -4, 'sobol: non-finite measure at input 6'),
        (dict(W_=changed(W, 9, np.inf)), -4, 'sobol: non-finite W'),
    ]
    for kw, code, text in cases:
        assert call(**kw) == code, text
        assert eng.last_error() == text
        assert all(np.all(o == 7.0) for o in outs), text
    with pytest.raises(FloatingPointError, match='non-finite W'):
        eng.sobol(kind, p0, p1, changed(W, 0, np.nan))
    with pytest.raises(ValueError, match='unknown output'):
        eng.sobol(kind, p0, p1, W, want=('S',))
    assert call() == 0                                             # a good call afterwards
    ref = R.sobol(params, D, S, M, kind, p0, p1, W)
    got = dict(zip(ALL, outs))
    assert all(v <= 1.0 for v in R.worst_ratio(got, ref, D).values())
    eng.close()
    from scfgp_amd.engine import HipEngine
    eng = HipEngine(D, S, M)                                       # no parameters: refused behind the argument checks
    assert eng.lib.scfgp_sobol(eng.ctx, ip(kind), dptr(p0), dptr(p1), dptr(W), 2, *[dptr(o) for o in outs]) == -1
    assert eng.last_error() == 'sobol: parameters not set'
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_training_state_survives(dtype):
    from scfgp_amd.engine import HipEngine
    D, S, M = 7, 12, 60
    params = synth.make_params(7, D, S, M, abc=(-1.0, 0.0, -1.0))
    X = synth.make_X(7, 1500, D)
    y = np.sin(3 * X[:, :1]) + 0.1 * synth.normal(10, 0, 1500)[:, None]
    eng = HipEngine(D, S, M, dtype=dtype); eng.set_params(params); eng.set_data(X, y)
    c0, g0, a0, L0 = eng.eval(want_grad=True)
    c0, g0, a0, L0 = float(c0), g0.copy(), a0.copy(), L0.copy()
    out = eng.sobol(*R.mixed_measure(D), eng.sample_weights(a0, L0, 40, seed=3), want=ALL)
    assert np.all(out['V'] > 0) and np.all(out['Vtot'] >= out['Vmain'] - 1e-12 * out['V'][:, None])
    c1, g1, a1, L1 = eng.eval(want_grad=True)
    assert float(c1) == c0 and np.array_equal(g1, g0) and np.array_equal(a1, a0) and np.array_equal(L1, L0)
    eng.close()


def _fitted_model():
    """a 4-column problem whose target depends on column 1 alone; column 2 is constant and dropped by the X scaler"""
    from scfgp_amd import SCFGP
    rng = np.random.default_rng(5)
    np.random.seed(5)
    X = rng.uniform(-2, 2, (400, 3))
    X = np.column_stack([X[:, :2], np.full(400, 4.0), X[:, 2:]])
    y = 3.0 + np.sin(2.0 * X[:, 1:2]) + 0.05 * rng.standard_normal((400, 1))
    model = SCFGP(sparsity=3, nfeats=12, device_scaler=True, X_scaling_method='min-max', y_scaling_method='normal')
    model.fit(X, y, max_iter=40,
              algo={'algo': 'adam', 'algo_params': {'learning_rate': 0.02, 'beta1': 0.9, 'beta2': 0.999, 'epsilon': 1e-8}})
    return model, X


@pytest.fixture(scope='module')
def fitted():
    return _fitted_model()


def test_facade_finds_the_input_that_matters(fitted):
    """Measured on the fit below: S = (0.0009, 0.967, 0, 0.0005), T = (0.023, 0.998, 0, 0.011); asserted with a wide margin"""
    model, X = fitted
    out = model.sobol(nsamples=24, seed=2)
    S, T = out['S'], out['T']
    print('facade sobol: S', np.round(S, 4), 'T', np.round(T, 4), 'V %.4f f0 %.4f' % (out['V'], out['f0']))
    assert S.shape == (4,) and T.shape == (4,) and S[2] == 0.0 and T[2] == 0.0           # the dropped column
    assert S[1] > 0.5 and S[1] > 5 * max(S[0], S[3]) and T[1] > 0.5
    assert np.all(T >= S - 1e-9) and abs(S.sum() - 1.0) < 0.5
    assert out['S_samples'].shape == (24, 4) and out['T_samples'].shape == (24, 4) and out['V_samples'].shape == (24,)
    assert np.all(out['S_q05'] <= out['S_q95']) and np.all(out['S_q05'][[0, 1, 3]] <= out['S_mean'][[0, 1, 3]])
    assert out['S_q05'][1] > 0.5
    # the training range in raw units through the min-max scaler IS the default measure
    lo, hi = X.min(0), X.max(0)
    b = model.sobol(bounds=np.column_stack((lo, hi)))
    assert np.allclose(b['S'], S, rtol=0, atol=1e-9) and np.allclose(b['T'], T, rtol=0, atol=1e-9)
    # normal inputs in raw units: mean through the transform, sd through its slope
    owner = model._owner('test')
    kind = np.array([1, 0, 0, 1]); p0 = np.array([0.3, lo[1], 0.0, -0.2]); p1 = np.array([0.5, hi[1], 0.0, 0.8])
    got = model.sobol(measure=(kind, p0, p1))
    sl = 1.0 / (hi - lo)[[0, 1, 3]]
    q0 = (p0 - lo)[[0, 1, 3]] * sl; q1 = np.where(kind[[0, 1, 3]] == 1, p1[[0, 1, 3]] * sl, (p1 - lo)[[0, 1, 3]] * sl)
    want = owner.engine.sobol(kind[[0, 1, 3]], q0, q1, model.alpha)
    assert np.allclose(got['S'][[0, 1, 3]], want['Vmain'][0] / want['V'][0], rtol=1e-9, atol=1e-12)
    with pytest.raises(ValueError, match='not both'):
        model.sobol(bounds=np.column_stack((lo, hi)), measure=(kind, p0, p1))
    from scfgp_amd.scaler import Scaler
    xs = Scaler('inv-normal'); xs.fit(X)
    with pytest.raises(ValueError, match="'inv-normal' is not affine"):
        owner.sobol_raw(None, lo, hi, xs, model.alpha)


def test_facade_nan_where_a_sample_has_no_variance(fitted):
    """point masses: every function is constant under the measure, so it has no indices"""
    model, X = fitted
    x = X[7]
    with np.errstate(all='raise'):
        out = model.sobol(bounds=np.column_stack((x, x)), nsamples=3)
    assert np.all(np.isnan(out['S'])) and np.all(np.isnan(out['T_samples'])) and abs(out['V']) < 1e-12


def test_facade_integral_is_the_quadrature_of_predict(fitted):
    model, X = fitted
    lo, hi = X.min(0), X.max(0)
    mean, sd = model.integral(bounds=np.column_stack((lo, hi)))
    x, w = np.polynomial.legendre.leggauss(24)
    ax = [0.5 * (lo[d] + hi[d]) + 0.5 * (hi[d] - lo[d]) * x for d in (0, 1, 3)]
    G = np.stack([g.ravel() for g in np.meshgrid(*ax, indexing='ij')], 1)
    Xq = np.column_stack([G[:, :2], np.full(len(G), 4.0), G[:, 2:]])
    wq = np.multiply.outer(np.multiply.outer(w, w), w).ravel() / 8.0
    mu = np.asarray(model.predict(Xq)[0]).reshape(-1)
    mu_scaled = np.asarray(model.y_scaler.forward_transform(mu.reshape(-1, 1))).reshape(-1)
    quad = float(wq @ mu_scaled)
    print('facade integral: %.12f (quadrature of predict %.12f), sd %.3e' % (mean, quad, sd))
    assert abs(mean - quad) <= 1e-8 * (1.0 + abs(quad)) and 0.0 < sd < 1.0
    m0, s0 = model.integral()                                      # the default measure is the same box
    assert abs(m0 - mean) <= 1e-12 * (1.0 + abs(mean)) and abs(s0 - sd) <= 1e-9 * sd
