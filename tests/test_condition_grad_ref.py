"""CPU tier of scfgp_condition_grad: the literal observation rows (tests/condition_grad_ref.py) against torch autograd of the literal
feature map and against the predictive mean's gradient; the algebra of the update (values and derivatives commute and compose; precise
derivative observations are interpolated); the vacuity of the GPU tier's bounds on its own inputs (a call that does nothing, and the
wrong forms of the rows); the coverage of the drawn precisions; and the C entry point's declaration (no GPU needed)."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from oracle import scfgp_oracle as O
from scfgp_amd import _lib
from scfgp_amd.scaler import Scaler
from tests import condition_grad_ref as R
from tests import condition_ref as CR
from tests import parity
from tests import pred_grad_ref as PG
from tests.test_gradcov_ref import _torch_features

CASES = [(3, 1, 5), (5, 4, 60), (8, 2, 20), (4, 3, 17)]          # S = 1; K = 128; odd J  (tests/test_predict_grad_ref.py)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def _small(D, S, M, seed, N=150, n=12):
    rng = np.random.default_rng(seed)
    params = O.init_params(D, S, M, rng)
    params[:3] = (-1.0, 0.0, -1.0)
    X = rng.uniform(0, 1, (N, D))
    y = np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((N, 1))
    _, alpha, Li = O.forward(X, y, params, S, M, gauss_hermite=False)
    Xn = rng.uniform(0, 1, (n, D))
    return params, alpha, Li, Xn, rng


@pytest.mark.parametrize('D,S,M', CASES)
def test_rows_equal_autograd_of_the_feature_map_and_the_mean_gradient(D, S, M):
    params, alpha, Li, Xn, rng = _small(D, S, M, 11 + D)
    n, K = len(Xn), 2 * (S + M)
    Psi, tg = R.rows(Xn, params, S, M, np.zeros((n, D)))
    assert Psi.shape == (n * D, K) and np.all(tg == 0)
    auto = np.stack([torch.autograd.functional.jacobian(lambda x: _torch_features(x, params, D, S, M), torch.tensor(x)).numpy()
                     for x in Xn])                                  # n x K x D
    assert rel(Psi.reshape(n, D, K), auto.transpose(0, 2, 1)) < 1e-12
    dmu = PG.predict_grad(Xn, alpha, Li, params, S, M)[2]
    assert rel((Psi @ np.asarray(alpha).reshape(-1)).reshape(n, D), dmu) < 1e-12
    assert rel(R.mean_grad(Xn, alpha, params, S, M), dmu) < 1e-12
    # the block layout: a value row first, then the derivative rows in the order of dims, scaled by sqrt(rho) and g
    dims = list(rng.permutation(D)[:max(1, D - 1)])
    rho = rng.choice([0.25, 1.0, 100.0], size=(n, len(dims))); G = rng.standard_normal((n, len(dims))); y = rng.standard_normal(n)
    g = rng.uniform(0.5, 2.0, (n, D))
    P2, t2 = R.rows(Xn, params, S, M, G, dims, rho, y, g)
    nb = len(dims) + 1
    assert P2.shape == (n * nb, K)
    assert rel(P2[0::nb], O.feature_map(Xn, params, D, S, M)) < 1e-15 and np.array_equal(t2[0::nb], y)
    for j, d in enumerate(dims):
        assert rel(P2[1 + j::nb], (np.sqrt(rho[:, j]) * g[:, d])[:, None] * auto[:, :, d]) < 1e-12
        assert np.allclose(t2[1 + j::nb], np.sqrt(rho[:, j]) * G[:, j], rtol=1e-15, atol=0)


@pytest.mark.parametrize('D,S,M', CASES)
def test_value_and_derivative_updates_commute_and_compose(D, S, M):
    params, alpha, Li, Xn, rng = _small(D, S, M, 23 + D)
    n = len(Xn)
    G = rng.standard_normal((n, D)); y = rng.standard_normal(n); rho = rng.choice(R.RHO_VALUES, size=(n, D))
    joint = R.condition_grad(Xn, G, alpha, Li, params, S, M, rho=rho, y=y)
    av, Lv = CR.condition(Xn, y, alpha, Li, params, S, M)
    value_first = R.condition_grad(Xn, G, av, Lv, params, S, M, rho=rho)
    ag, Lg = R.condition_grad(Xn, G, alpha, Li, params, S, M, rho=rho)
    grad_first = CR.condition(Xn, y, ag, Lg, params, S, M)
    for other in (value_first, grad_first):
        assert rel(other[0], joint[0]) < 1e-10 and rel(other[1], joint[1]) < 1e-10
    assert rel(joint[0], alpha) > 1e-3                              # the observations did move the posterior


def test_precise_derivative_observations_are_interpolated():
    """D <= S: every phase is x l_F [I | r_F^T] + offset, so the model's gradients span rank(l_F) = min(D, S) directions and D arbitrary
    derivatives per point can be met only then.  What is left of the misfit is (I + rho Psi A^-1 Psi^T)^-1 (G - Psi alpha), so the fit
    that is updated is a weak one (8 rows) and the points are few (2): 2e-8 .. 5e-8 over seeds 5, 6, 7 where a fit of 150 rows leaves
    3e-4."""
    D, S, M = 2, 3, 40
    params, alpha, Li, Xn, rng = _small(D, S, M, 5, N=8, n=2)
    G = rng.standard_normal((len(Xn), D))
    a1, _ = R.condition_grad(Xn, G, alpha, Li, params, S, M, rho=np.full(G.shape, 1e8))
    assert rel(R.mean_grad(Xn, a1, params, S, M), G) < 1e-6
    assert rel(R.mean_grad(Xn, alpha, params, S, M), G) > 0.1


# ---- the GPU tier's own inputs -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gpu_case(i):
    D, S, M, N0, n, dims = R.SHAPES[i]
    p = R.problem(D, S, M, N0, n, dims)
    _, a0, L0 = O.forward(p['X0'], p['y0'], p['params'], S, M, gauss_hermite=False)
    good = R.condition_grad(p['Xn'], p['G'], a0, L0, p['params'], S, M, dims=dims, rho=p['rho'], y=p['yn'])
    return p, a0, L0, good


def _moved(bad, good):
    """the distance of two pairs of factors in fp32 bounds of the GPU tier"""
    return max(parity.alpha_ratio(bad[0], good[0], 'f32'), parity.li_ratio(bad[1], good[1], 'f32'))


@pytest.mark.parametrize('i', range(len(R.SHAPES)))
def test_a_call_that_does_nothing_fails_the_gpu_bound(i):
    D, S, M, N0, n, dims = R.SHAPES[i]
    p, a0, L0, good = _gpu_case(i)
    assert parity.alpha_ratio(a0, good[0], 'f32') > 1.0
    # and in each of the tier's four forms of the call (with and without values, with and without rho)
    for y in (None, p['yn']):
        for rho in (None, p['rho']):
            a1, _ = R.condition_grad(p['Xn'], p['G'], a0, L0, p['params'], S, M, dims=dims, rho=rho, y=y)
            assert parity.alpha_ratio(a0, a1, 'f32') > 1.0, (R.SHAPES[i], y is not None, rho is not None)


# the single-row shape is left out: one observation row moves the factors by a few fp32 bounds in all, so no form of that row is 100
# bounds away from another; its row is checked through the shapes around it, which run the same code
# and 'sorted_dims' runs where dims are not in order already
def _unsorted(k):
    return R.SHAPES[k][5] is not None and list(R.SHAPES[k][5]) != sorted(R.SHAPES[k][5])


@pytest.mark.parametrize('i,mutate', [(k, m) for k in range(len(R.SHAPES)) if R.SHAPES[k][4] > 1 for m in R.MUTATIONS
                                      if m != 'sorted_dims' or _unsorted(k)])
def test_wrong_rows_move_the_reference_far_beyond_the_gpu_bound(i, mutate):
    D, S, M, N0, n, dims = R.SHAPES[i]
    p, a0, L0, good = _gpu_case(i)
    bad = R.condition_grad(p['Xn'], p['G'], a0, L0, p['params'], S, M, dims=dims, rho=p['rho'], y=p['yn'], mutate=mutate)
    r = _moved(bad, good)
    print(mutate, R.SHAPES[i], r)
    assert r > 100.0


@pytest.mark.parametrize('mutate', R.RAW_MUTATIONS)
@pytest.mark.parametrize('xalgo', Scaler.algos)
def test_wrong_scaler_factors_move_the_reference_far_beyond_the_gpu_bound(xalgo, mutate):
    q = R.raw_problem(xalgo)
    S, M = q['S'], q['M']
    cols = q['xs'].data['cols']
    Xs = q['xs'].forward_transform(q['Xr']); g = q['xs'].forward_derivative(q['Xr'])
    assert np.allclose(g, PG.x_scaler_deriv(q['xs'], q['Xr']), rtol=1e-14, atol=0)
    G = (q['dY'] * q['ys'].forward_derivative(q['yr']))[:, cols]
    rho = q['rho'][:, cols]
    good = R.condition_grad(Xs, G, q['alpha'], q['Li'], q['params'], S, M, rho=rho, g=g)
    bad = R.condition_grad(Xs, G, q['alpha'], q['Li'], q['params'], S, M, rho=rho, g=g, mutate=mutate)
    r = _moved(bad, good)
    print(mutate, xalgo, r)
    assert r > 100.0


@pytest.mark.parametrize('i', range(len(R.SHAPES)))
def test_drawn_precisions_cover_zero_without_emptying_a_point(i):
    D, S, M, N0, n, dims = R.SHAPES[i]
    rho = R.problem(D, S, M, N0, n, dims)['rho']
    assert set(np.unique(rho)) <= set(R.RHO_VALUES)
    assert not np.any(np.all(rho == 0, axis=1))                     # no point has all of its precisions 0
    if rho.size >= 100:                                             # a share is a share of something: the small shapes hold too few draws
        assert 0.05 <= np.mean(rho == 0) <= 0.25, np.mean(rho == 0)


def test_unit_rho_brings_a_derivative_row_to_the_length_of_a_value_row():
    D, S, M = 5, 4, 60
    params, alpha, Li, Xn, rng = _small(D, S, M, 3)
    n = len(Xn)
    dims = [4, 1]
    Psi, _ = R.rows(Xn, params, S, M, np.zeros((n, 2)), dims, np.tile(R.unit_rho(params, D, S, M, dims), (n, 1)), np.zeros(n))
    norms = np.linalg.norm(Psi, axis=1).reshape(n, 3)
    assert np.allclose(norms, norms[:, :1], rtol=1e-12, atol=0)


def test_scaler_forward_derivative_is_the_derivative():
    rng = np.random.default_rng(2)
    X = np.column_stack([rng.uniform(0.5, 3.0, 300), rng.gamma(2.0, 1.0, 300), np.full(300, 2.5)])
    for algo in Scaler.algos:
        s = Scaler(algo); s.fit(X)
        h = 1e-6
        fd = (s.forward_transform(X[:20] + h) - s.forward_transform(X[:20] - h)) / (2 * h)
        assert rel(s.forward_derivative(X[:20]), fd) < 1e-7, algo
        assert s.affine == (algo in ('min-max', 'normal'))


def test_condition_grad_entry_point_declared_exported_and_checked_without_gpu():
    """scfgp_condition_grad is in the header, the library and the binding table with the documented argument types, and refuses bad
    arguments before touching a device or an output."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'include', 'scfgp_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    cd = r'const double\s*\*\s*'
    assert re.search(r'\bint\s+scfgp_condition_grad\s*\(\s*scfgp_ctx\s*\*\s*ctx,\s*' + cd + r'Xn,\s*int64_t n,\s*const int32_t\s*\*\s*dims,'
                     r'\s*int nd,\s*' + cd + r'Gn,\s*' + cd + r'rho,\s*' + cd + r'yn,\s*' + cd + r'alpha,\s*' + cd + r'Li,\s*int mode,'
                     r'\s*double\s*\*\s*alpha_out,\s*double\s*\*\s*Li_out\s*\)', header)
    comment = [c for c in re.findall(r'/\*.*?\*/', text, flags=re.S) if 'absorbing derivative observations' in c]
    assert len(comment) == 1
    for promise in ('exactly zero above the diagonal', 'may alias', 'training state of the context survives', 'bit for bit',
                    'rho = 0', 'device memory does not grow with n', 'Out of scope'):
        assert promise in comment[0], promise
    dp = _lib._c_double_p
    assert _lib.SIGNATURES['scfgp_condition_grad'] == (ctypes.c_int, [ctypes.c_void_p, dp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int32),
                                                                      ctypes.c_int, dp, dp, dp, dp, dp, ctypes.c_int, dp, dp])
    lib = _lib.load()
    fn = lib.scfgp_condition_grad
    D, S, M = 3, 2, 5
    K = 2 * (S + M)
    X = np.zeros((4, D)); G = np.zeros((4, D)); alpha = np.zeros(K); Li = np.eye(K)
    ao, Lo = np.full(K, 7.0), np.full((K, K), 7.0)
    p = _lib.dptr
    assert fn(None, p(X), 4, None, D, p(G), None, None, p(alpha), p(Li), 0, p(ao), p(Lo)) == -1
    ctx = ctypes.c_void_p()
    lib.scfgp_create(ctypes.byref(ctx), D, S, M, 0, 0, None)        # fails on a GPU-less box but hands back its context
    assert ctx.value
    try:
        assert fn(ctx, None, 4, None, D, p(G), None, None, p(alpha), p(Li), 0, p(ao), p(Lo)) == -1
        assert lib.scfgp_last_error(ctx) == b'condition_grad: bad arguments'
        assert fn(ctx, p(X), 4, None, D, p(G), None, None, p(alpha), p(Li), 0, p(ao), p(Lo)) == -1
        assert lib.scfgp_last_error(ctx) == b'condition_grad: parameters not set'
        assert np.all(ao == 7.0) and np.all(Lo == 7.0)
    finally:
        lib.scfgp_destroy(ctx)
