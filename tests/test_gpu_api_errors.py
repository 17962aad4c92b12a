"""The weight checks of the eight entry points that take weights, behind "parameters not set": one context of (D, S, M) = (3, 2, 4) with
parameters set and a pool of 5 rows.  Every case asserts the exception class and the whole message (the engine's "<call>: " in front of
the library's text, written out here); every case is refused on the host, before any device work.  The checks that stand before
"parameters not set" are in tests/test_api_errors_cpu.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, S, M, T = 3, 2, 4, 5
K = 2 * (S + M)
nan, inf = float('nan'), float('inf')
NEG_FIRST = [1.0, -1.0, nan, 1.0, 1.0]          # the negative row wins, at row 1
NAN_FIRST = [nan, -1.0, 1.0, 1.0, 1.0]          # it still wins behind a non-finite weight (predict_gradcov names weight 0)
INF = [1.0, inf, 1.0, 1.0, 1.0]
ZEROS = [0.0] * 5
ONE = [0.0, 1.0, 0.0, 0.0, 0.0]
NONFINITE = {'sample_argmax': 'non-finite rows, weights or factors', 'acquire': 'non-finite par, fstar or weights',
             'acquire_kg': 'non-finite nodes or weights', 'predict_pd': 'non-finite weights',
             'select': 'non-finite rows, weights or factors', 'select_iv': 'non-finite rows, weights or factors',
             'select_qei': 'non-finite best, xi or weights'}
POOL = ('sample_argmax', 'acquire', 'acquire_kg', 'predict_pd')          # "no row has a positive weight"
PICKS = ('select', 'select_iv', 'select_qei')                            # "m = 2 but only ... rows have a positive weight"


@pytest.fixture(scope='module')
def ctx():
    from scfgp_amd import synth
    from scfgp_amd.engine import HipEngine
    rng = np.random.default_rng(3)
    eng = HipEngine(D, S, M, dtype='f64')
    eng.set_params(synth.make_params(11, D, S, M, abc=(-1.0, 0.0, -1.0)))
    X = synth.make_X(3, T, D)
    Li = 0.02 * (np.tril(rng.standard_normal((K, K))) / np.sqrt(K) + np.eye(K))
    alpha = rng.standard_normal(K) / np.sqrt(K)
    yield eng, X, alpha, Li
    eng.close()


def call(ctx, name, w, m=2, **kw):
    eng, X, alpha, Li = ctx
    w = np.array(w)
    if name == 'sample_argmax':
        return eng.sample_argmax(X, alpha, Li, 2, w=w)
    if name == 'acquire':
        return eng.acquire(X, alpha, Li, 'ucb', beta=kw.get('beta', 1.0), w=w)
    if name == 'acquire_kg':
        return eng.acquire_kg(X, alpha, Li, w=w)
    if name == 'predict_gradcov':
        return eng.predict_gradcov(X, alpha, Li, w=w, want=('asub',))
    if name == 'predict_pd':
        return eng.predict_pd(X, alpha, Li, [0], np.zeros((1, 2)), w=w)
    if name == 'select':
        return eng.select(X, Li, m, w=w)
    if name == 'select_iv':
        return eng.select_iv(X, Li, m, w=w, wr=kw.get('wr'))
    if name == 'select_qei':
        return eng.select_qei(X, alpha, Li, m, 2, kw.get('best', 0.0), w=w)
    raise KeyError(name)


def refused(ctx, name, w, cls, text, **kw):
    with pytest.raises(cls) as e:
        call(ctx, name, w, **kw)
    assert type(e.value) is cls
    assert str(e.value) == '%s: %s: %s' % (name, name, text)


@pytest.mark.parametrize('name', POOL + PICKS)
@pytest.mark.parametrize('w', [NEG_FIRST, NAN_FIRST], ids=['neg_first', 'nan_first'])
def test_negative_row_wins(ctx, name, w):
    refused(ctx, name, w, ValueError, 'negative weight at row 1')


@pytest.mark.parametrize('name', POOL + PICKS)
def test_nonfinite_weight(ctx, name):
    refused(ctx, name, INF, FloatingPointError, NONFINITE[name])


@pytest.mark.parametrize('name', POOL)
def test_no_positive_weight(ctx, name):
    refused(ctx, name, ZEROS, ValueError, 'no row has a positive weight')


@pytest.mark.parametrize('name', PICKS)
@pytest.mark.parametrize('w,n', [(ZEROS, 0), (ONE, 1)], ids=['zeros', 'one'])
def test_too_few_eligible_rows(ctx, name, w, n):
    refused(ctx, name, w, ValueError, 'm = 2 but only %d rows have a positive weight' % n)


@pytest.mark.parametrize('w,text', [(NEG_FIRST, 'weight 1 is negative or not finite'), (NAN_FIRST, 'weight 0 is negative or not finite'),
                                    (INF, 'weight 1 is negative or not finite'), (ZEROS, 'the weights sum to zero')],
                         ids=['neg_first', 'nan_first', 'inf', 'zeros'])
def test_predict_gradcov_with_asub(ctx, w, text):
    refused(ctx, 'predict_gradcov', w, ValueError, text)


@pytest.mark.parametrize('wr,cls,text', [(NEG_FIRST, ValueError, 'negative reference weight at row 1'),
                                         (NAN_FIRST, ValueError, 'negative reference weight at row 1'),
                                         (INF, FloatingPointError, 'non-finite rows, weights or factors'),
                                         (ZEROS, ValueError, 'no reference row has a positive weight')],
                         ids=['neg_first', 'nan_first', 'inf', 'zeros'])
def test_select_iv_reference_weights(ctx, wr, cls, text):
    refused(ctx, 'select_iv', [1.0] * 5, cls, text, wr=np.array(wr))


def test_select_iv_reference_weights_pass_then_pool_weights_refuse(ctx):
    refused(ctx, 'select_iv', ONE, ValueError, 'm = 2 but only 1 rows have a positive weight', wr=np.array(ONE))


def test_select_iv_nonfinite_pool_weight_silences_the_reference_count(ctx):
    # a non-finite w: "no reference row has a positive weight" is not reported, the shared flag is
    refused(ctx, 'select_iv', INF, FloatingPointError, 'non-finite rows, weights or factors', wr=np.array(ZEROS))


def test_negative_weight_is_reported_before_a_nonfinite_parameter(ctx):
    refused(ctx, 'acquire', NEG_FIRST, ValueError, 'negative weight at row 1', beta=nan)
    refused(ctx, 'select_qei', NEG_FIRST, ValueError, 'negative weight at row 1', best=nan)
    refused(ctx, 'acquire', [1.0] * 5, FloatingPointError, 'non-finite par, fstar or weights', beta=nan)
    refused(ctx, 'select_qei', [1.0] * 5, FloatingPointError, 'non-finite best, xi or weights', best=nan)


def test_y_scaler_is_asked_for_behind_the_x_scaler():
    from scfgp_amd import synth
    from scfgp_amd.engine import HipEngine
    from scfgp_amd.scaler import Scaler
    eng = HipEngine(D, S, M, dtype='f64')
    try:
        X = synth.make_X(3, T, D)
        xs = Scaler('normal'); xs.fit(X)
        eng.set_x_scaler(xs)
        alpha, Li = np.zeros(K), np.eye(K)
        for name, fn in (('sample', lambda: eng.sample(X, alpha, Li, 2, mode='y')),
                         ('sample_argmax', lambda: eng.sample_argmax(X, alpha, Li, 2, mode='y')),
                         ('sample_grad', lambda: eng.sample_grad(X, np.zeros((K, 2)), mode='y'))):
            with pytest.raises(ValueError) as e:
                fn()
            assert str(e.value) == '%s: %s: no y scaler set' % (name, name)
    finally:
        eng.close()
