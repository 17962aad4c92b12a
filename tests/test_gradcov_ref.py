"""CPU tier of scfgp_predict_gradcov: the closed form of the gradient's posterior (tests/gradcov_ref.py) against torch autograd of the
literal feature map, finite differences of the oracle's feature map and the mixed second difference of the posterior covariance; the
latent form the device runs against the dense one; the active-subspace matrix; the vacuity of the GPU tier's bounds (mutations); and
the C entry point's declaration and argument checks (no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import scfgp_oracle as O
from scfgp_amd import _lib
from scfgp_amd.scaler import Scaler
from tests import gradcov_ref as R
from tests import pred_cov_ref as PC
from tests import pred_grad_ref as PG

CASES = [(3, 1, 5), (5, 4, 60), (8, 2, 20), (4, 3, 17)]          # S = 1; K = 128; odd J  (tests/test_predict_grad_ref.py)
F32_BOUND = 6e-6                                                  # the GPU tier's fp32 bound on dvar, dcov, asub


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def _problem(D, S, M, seed, N=150, T=12):
    rng = np.random.default_rng(seed)
    params = O.init_params(D, S, M, rng)
    params[:3] = (-1.0, 0.0, -1.0)
    X = rng.uniform(0, 1, (N, D))
    y = np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((N, 1))
    _, alpha, Li = O.forward(X, y, params, S, M, gauss_hermite=False)
    return params, alpha, Li, rng.uniform(0, 1, (T, D))


def _torch_features(x, params, D, S, M):
    """SCFGP/SCFGP.py:139-142 restated in torch float64 for one row x (D,)"""
    p = torch.tensor(params)
    t = 3
    l_F = p[t:t + D * S].reshape(D, S); t += D * S
    r_F = p[t:t + M * S].reshape(M, S); t += M * S
    F = l_F @ r_F.T
    l_P = p[t:t + S].reshape(1, S); t += S
    P = p[t:t + M].reshape(1, M)
    FFs = torch.cat((x[None, :] @ l_F + l_P - l_F.mean(0)[None, :], x[None, :] @ F + P - F.mean(0)[None, :]), 1)
    return (torch.exp(p[1]) * np.sqrt(2. / M) * torch.cat((torch.cos(FFs), torch.sin(FFs)), 1))[0]


@pytest.mark.parametrize('D,S,M', CASES)
def test_jacobian_equals_autograd_finite_differences_and_predict_grad(D, S, M):
    params, alpha, Li, Xs = _problem(D, S, M, 11 + D)
    J = R.jacobian(Xs, params, S, M)
    assert J.shape == (len(Xs), 2 * (S + M), D)
    auto = np.stack([torch.autograd.functional.jacobian(lambda x: _torch_features(x, params, D, S, M), torch.tensor(x)).numpy()
                     for x in Xs])
    assert rel(J, auto) < 1e-12
    h = 1e-5
    fd = np.empty_like(J)
    for d in range(D):
        e = np.zeros(D); e[d] = h
        fd[:, :, d] = (O.feature_map(Xs + e, params, D, S, M) - O.feature_map(Xs - e, params, D, S, M)) / (2 * h)
    assert rel(J, fd) < 1e-6
    m, _ = R.gradcov(Xs, alpha, Li, params, S, M)
    assert rel(m, PG.predict_grad(Xs, alpha, Li, params, S, M)[2]) < 1e-12


@pytest.mark.parametrize('D,S,M', CASES)
def test_covariance_equals_mixed_second_difference_of_pred_cov(D, S, M):
    """Sigma_t[d][e] = d^2 k(x, x') / dx_d dx'_e at x = x' = x_t, k the posterior covariance of the function values.  The central
    scheme [k(+,+) - k(+,-) - k(-,+) + k(-,-)] / 4h^2 has truncation error O(h^2) and rounding error O(eps |k| / h^2); measured against
    the closed form on these four cases its relative error is 1.7e-4 .. 5e-5 at h = 1e-2, falls a hundredfold per decade of h down to
    1.7e-8 .. 6e-9 at h = 1e-4 and rises again to 4e-7 at h = 1e-5.  Step 1e-4, bound 2e-7: ten times the worst case measured.  A
    wrong sign, a factor 1/2 or a missing kappa are errors of order 1."""
    params, alpha, Li, Xs = _problem(D, S, M, 11 + D, T=6)
    _, Sig = R.gradcov(Xs, alpha, Li, params, S, M)
    h = 1e-4
    k = lambda a, b: PC.pred_cov(a[None], Li, params, S, M, Xb=b[None])[0, 0]
    fd = np.empty_like(Sig)
    for t, x in enumerate(Xs):
        for d in range(D):
            for e in range(D):
                ed = np.zeros(D); ed[d] = h
                ee = np.zeros(D); ee[e] = h
                fd[t, d, e] = (k(x + ed, x + ee) - k(x + ed, x - ee) - k(x - ed, x + ee) + k(x - ed, x - ee)) / (4 * h * h)
    err = rel(fd, Sig)
    print('mixed second difference', (D, S, M), err)
    assert err < 2e-7


@pytest.mark.parametrize('D,S,M', [(9, 4, 11), (6, 6, 10), (3, 7, 5), (70, 5, 60), (1, 2, 2)])       # D > S, D = S, D < S
def test_latent_form_equals_dense_form(D, S, M):
    params, alpha, Li = R.synthetic(D, S, M)
    Xs = R.points(D, 23)
    g = 0.5 + R.points(D + 1, 23)[:, :D]
    Q, P = R.basis(params, D, S, M)
    assert Q.shape == (S + M, min(D, S)) and P.shape == (D, min(D, S))
    assert rel(P @ Q.T, PG.fall(params, D, S, M)) < 1e-14
    for gg in (None, g):
        m0, S0 = R.gradcov(Xs, alpha, Li, params, S, M, g=gg)
        m1, S1 = R.gradcov_latent(Xs, alpha, Li, params, S, M, g=gg)
        assert rel(m1, m0) < 1e-12 and rel(S1, S0) < 1e-12


@pytest.mark.parametrize('D,S,M', [(9, 4, 11), (3, 7, 5)])
def test_asub_is_symmetric_psd_with_the_right_trace(D, S, M):
    params, alpha, Li = R.synthetic(D, S, M)
    Xs = R.points(D, 40)
    m, Sig = R.gradcov(Xs, alpha, Li, params, S, M)
    for w in (None, np.r_[np.linspace(0.0, 2.0, 30), np.zeros(10)]):
        A = R.asub(m, Sig, w)
        assert np.allclose(A, A.T, rtol=0, atol=1e-15 * np.abs(A).max())
        lam = np.linalg.eigvalsh(0.5 * (A + A.T))
        assert lam[0] >= -1e-12 * np.trace(A)
        ww = np.ones(40) if w is None else w
        tr = float((ww * ((m ** 2).sum(1) + np.trace(Sig, axis1=1, axis2=2))).sum() / ww.sum())
        assert abs(np.trace(A) - tr) < 1e-12 * tr


@pytest.mark.parametrize('D,S,M', R.GEOMETRIES)
@pytest.mark.parametrize('mutate', ['no_minus', 'swap_halves', 'no_kappa'])
def test_mutations_move_the_reference_far_beyond_the_gpu_bound(D, S, M, mutate):
    """vacuity check of the GPU tier's parity bounds on its own inputs: each wrong form is at least 100 fp32 bounds away"""
    params, alpha, Li = R.synthetic(D, S, M)
    Xs = R.points(D)[:64]
    m, Sig = R.gradcov(Xs, alpha, Li, params, S, M)
    _, bad = R.gradcov(Xs, alpha, Li, params, S, M, mutate=mutate)
    dv = rel(np.diagonal(bad, axis1=1, axis2=2), np.diagonal(Sig, axis1=1, axis2=2))
    dc, da = rel(bad, Sig), rel(R.asub(m, bad), R.asub(m, Sig))
    print(mutate, (D, S, M), dv, dc, da)
    assert min(dv, dc, da) > 100 * F32_BOUND


@pytest.mark.parametrize('xalgo', Scaler.algos)
def test_one_sided_scaler_factor_moves_the_reference_far_beyond_the_gpu_bound(xalgo):
    (D, S, M), xs, (params, alpha, Li), Xr = R.raw_problem(xalgo)
    Xs = xs.forward_transform(Xr)
    g = PG.x_scaler_deriv(xs, Xr)
    m, Sig = R.gradcov(Xs, alpha, Li, params, S, M, g=g)
    _, bad = R.gradcov(Xs, alpha, Li, params, S, M, g=g, mutate='one_sided_g')
    dv = rel(np.diagonal(bad, axis1=1, axis2=2), np.diagonal(Sig, axis1=1, axis2=2))
    assert min(dv, rel(bad, Sig), rel(R.asub(m, bad), R.asub(m, Sig))) > 100 * F32_BOUND


def test_predict_gradcov_entry_point_declared_exported_and_checked_without_gpu():
    """scfgp_predict_gradcov is in the header, the library and the binding table with the documented argument types, and refuses bad
    arguments before touching a device or an output."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'scfgp_hip.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+scfgp_predict_gradcov\s*\(\s*scfgp_ctx\s*\*\s*ctx,\s*const double\s*\*\s*Xs,\s*int64_t T,\s*const double\s*\*\s*w,'
                     r'\s*const double\s*\*\s*alpha,\s*const double\s*\*\s*Li,\s*int mode,\s*double\s*\*\s*dmu,\s*double\s*\*\s*dvar,'
                     r'\s*double\s*\*\s*dcov,\s*double\s*\*\s*asub\s*\)', header)
    dp = _lib._c_double_p
    assert _lib.SIGNATURES['scfgp_predict_gradcov'] == (ctypes.c_int, [ctypes.c_void_p, dp, ctypes.c_int64, dp, dp, dp, ctypes.c_int,
                                                                       dp, dp, dp, dp])
    lib = _lib.load()
    fn = lib.scfgp_predict_gradcov
    D, S, M = 3, 2, 5
    K = 2 * (S + M)
    Xs = np.zeros((4, D)); alpha = np.zeros(K); Li = np.eye(K); w = np.ones(4)
    out = [np.full((4, D), 7.0), np.full((4, D), 7.0), np.full((4, D, D), 7.0), np.full((D, D), 7.0)]
    p = _lib.dptr
    o = [p(a) for a in out]
    assert fn(None, p(Xs), 4, None, p(alpha), p(Li), 0, *o) == -1
    ctx = ctypes.c_void_p()
    lib.scfgp_create(ctypes.byref(ctx), D, S, M, 0, 0, None)        # fails on a GPU-less box but hands back its context
    assert ctx.value
    try:
        for T in (0, -3):
            assert fn(ctx, p(Xs), T, None, p(alpha), p(Li), 0, *o) == -1
        for mode in (-1, 2, 7):
            assert fn(ctx, p(Xs), 4, None, p(alpha), p(Li), mode, *o) == -1
        assert fn(ctx, None, 4, None, p(alpha), p(Li), 0, *o) == -1
        assert b'bad arguments' in lib.scfgp_last_error(ctx)
        assert fn(ctx, p(Xs), 4, p(w), p(alpha), p(Li), 0, None, None, None, None) == -1
        assert b'no output' in lib.scfgp_last_error(ctx)
        assert fn(ctx, p(Xs), 4, None, p(alpha), p(Li), 1, *o) == -1
        assert b'scaler' in lib.scfgp_last_error(ctx)
        assert fn(ctx, p(Xs), 4, None, p(alpha), p(Li), 0, *o) == -1                   # parameters not set
        assert b'parameters' in lib.scfgp_last_error(ctx)
        assert all(np.all(a == 7.0) for a in out)
    finally:
        lib.scfgp_destroy(ctx)
