"""CPU tier of scfgp_amd.ascent.ascend: the batched projected-gradient ascent on the numpy closed form of the sample functions
(tests/sample_grad_ref.py) and on quadratics with known maximisers (no GPU needed)."""
import numpy as np
import pytest

from oracle import scfgp_oracle as O
from scfgp_amd.ascent import ascend
from tests import sample_grad_ref as R
from tests import sample_ref as SR

D, S, M, NSAMP, SEED = 2, 1, 6, 16, 3
MAX_ITER, GTOL = 60, 1e-6


@pytest.fixture(scope='module')
def model():
    rng = np.random.default_rng(SEED)
    params = O.init_params(D, S, M, rng)
    params[:3] = (-1.0, 0.0, -1.0)
    X = rng.uniform(0, 1, (60, D))
    y = np.sin(3 * X.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((60, 1))
    _, alpha, Li = O.forward(X, y, params, S, M, gauss_hermite=False)
    W = SR.weights(alpha, Li, SR.kappa(params), NSAMP, SEED)
    g = np.linspace(0.0, 1.0, 12)
    pool = np.stack(np.meshgrid(g, g, indexing='ij'), -1).reshape(-1, D)
    F = O.feature_map(pool, params, D, S, M) @ W                # (144, NSAMP)
    calls = []

    def fg(Xq, sidx):
        calls.append(len(sidx))
        return R.sample_grad(Xq, W, sidx, params, S, M)
    return dict(params=params, W=W, pool=pool, F=F, fg=fg, calls=calls)


@pytest.mark.parametrize('minimize', [False, True])
def test_ascent_on_the_sample_functions(model, minimize):
    F, pool, fg = model['F'], model['pool'], model['fg']
    start = F.argmin(0) if minimize else F.argmax(0)
    sidx = np.arange(NSAMP)
    X0 = pool[start]
    v0, _ = fg(X0, sidx)
    del model['calls'][:]
    X, val, conv, n_calls = ascend(fg, X0, sidx, 0.0, 1.0, minimize=minimize, max_iter=MAX_ITER, gtol=GTOL)
    assert n_calls == len(model['calls'])                      # every evaluation is one batched call ...
    assert model['calls'][0] == NSAMP and max(model['calls']) <= NSAMP      # ... on the rows still active
    assert X.shape == (NSAMP, D) and val.shape == (NSAMP,) and conv.shape == (NSAMP,) and conv.dtype == bool
    assert np.all(val <= v0) if minimize else np.all(val >= v0)
    assert np.all(X >= 0.0) and np.all(X <= 1.0)
    vr, gr = R.sample_grad(X, model['W'], sidx, model['params'], S, M)
    assert np.array_equal(vr, val)                             # the returned value is fg's at the returned point
    pg = R.projected_gradient_norm(X, gr, 0.0, 1.0, minimize=minimize)
    assert np.all(pg[conv] <= GTOL * np.maximum(1.0, np.abs(vr[conv])))
    assert conv.sum() >= NSAMP / 2                             # at least half of the rows at max_iter = 60


def test_ascent_is_deterministic_and_rows_do_not_interact(model):
    F, pool, fg = model['F'], model['pool'], model['fg']
    sidx = np.arange(NSAMP)
    X0 = pool[F.argmax(0)]
    Xa, va, ca, _ = ascend(fg, X0, sidx, 0.0, 1.0, max_iter=MAX_ITER, gtol=GTOL)
    Xb, vb, cb, _ = ascend(fg, X0, sidx, 0.0, 1.0, max_iter=MAX_ITER, gtol=GTOL)
    assert np.array_equal(Xa, Xb) and np.array_equal(va, vb) and np.array_equal(ca, cb)
    # a row's trajectory is its own: on a quadratic (exact arithmetic per row) a subset of the rows takes the same steps
    centre = np.linspace(0.1, 0.9, 10).reshape(5, 2); scale = np.linspace(1.0, 9.0, 10).reshape(5, 2)
    q = _quadratic(centre, scale)
    Xq, vq, cq, _ = ascend(q, np.full((5, 2), 0.5), np.arange(5), 0.0, 1.0)
    sub = np.array([4, 1])
    Xs, vs, cs, _ = ascend(q, np.full((2, 2), 0.5), sub, 0.0, 1.0)
    assert np.array_equal(Xs, Xq[sub]) and np.array_equal(vs, vq[sub]) and np.array_equal(cs, cq[sub])


def _quadratic(centre, scale):
    centre = np.asarray(centre, np.float64); scale = np.asarray(scale, np.float64)

    def fg(X, sidx):
        d = X - centre[sidx]
        return 2.0 - 0.5 * (scale[sidx] * d * d).sum(1), -scale[sidx] * d
    return fg


def test_quadratic_with_known_maximiser_inside_and_on_the_boundary():
    centre = np.array([[0.3, 0.6, 0.5], [1.4, 0.2, -0.3], [0.9, 0.9, 0.1]])     # row 1: outside the box in two coordinates
    scale = np.array([[1.0, 10.0, 3.0], [2.0, 0.5, 4.0], [100.0, 1.0, 1.0]])
    fg = _quadratic(centre, scale)
    X0 = np.full((3, 3), 0.5)
    X, val, conv, n_calls = ascend(fg, X0, np.arange(3), 0.0, 1.0, max_iter=200, gtol=1e-9)
    expect = np.clip(centre, 0.0, 1.0)                           # separable: the box maximiser is the clipped centre
    assert conv.all()
    assert np.abs(X - expect).max() < 1e-6
    assert np.allclose(val, fg(expect, np.arange(3))[0], rtol=0, atol=1e-10)
    # minimising the negated function finds the same points
    neg = lambda Xq, s: tuple(-a for a in fg(Xq, s))
    Xm, vm, cm, _ = ascend(neg, X0, np.arange(3), 0.0, 1.0, minimize=True, max_iter=200, gtol=1e-9)
    assert cm.all() and np.abs(Xm - expect).max() < 1e-6 and np.allclose(vm, -val, rtol=0, atol=1e-10)


def test_bad_arguments():
    fg = _quadratic(np.zeros((1, 2)), np.ones((1, 2)))
    with pytest.raises(ValueError):
        ascend(fg, np.array([[2.0, 0.5]]), [0], 0.0, 1.0)        # a start outside the box
    with pytest.raises(ValueError):
        ascend(fg, np.array([[0.5, 0.5]]), [0, 0], 0.0, 1.0)     # sidx of the wrong length
    with pytest.raises(ValueError):
        ascend(fg, np.array([[0.5, 0.5]]), [0], 1.0, 0.0)
