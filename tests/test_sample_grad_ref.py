"""CPU tier of scfgp_sample_grad: the closed-form values and input gradients of sample functions (tests/sample_grad_ref.py) against
torch autograd of the literal graph f = phi(x)^T w and against central differences of tests/sample_ref.py, its agreement with the mean
gradient of tests/pred_grad_ref.py, two mutations that the autograd comparison must catch, and the C entry point's argument checks
(no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import scfgp_oracle as O
from scfgp_amd import _lib
from tests import pred_grad_ref as G
from tests import sample_grad_ref as R
from tests import sample_ref as SR

CASES = [(3, 1, 5), (5, 4, 60), (8, 2, 20), (4, 3, 17)]          # S = 1; K = 128; odd J  (those of test_predict_grad_ref)
NSAMP = 7


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def _problem(D, S, M, seed, N=150, T=40):
    rng = np.random.default_rng(seed)
    params = O.init_params(D, S, M, rng)
    params[:3] = (-1.0, 0.0, -1.0)
    X = rng.uniform(0, 1, (N, D))
    y = np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((N, 1))
    _, alpha, Li = O.forward(X, y, params, S, M, gauss_hermite=False)
    W = SR.weights(alpha, Li, SR.kappa(params), NSAMP, seed)
    return params, alpha, Li, W, rng.uniform(0, 1, (T, D)), rng.integers(0, NSAMP, T)


def _torch_literal(Xs, Wrows, params, S, M):
    """f_t = phi(x_t)^T w_t on the literal feature graph (SCFGP/SCFGP.py:139-142) in torch float64; returns f and its autograd
    gradient in Xs.  Wrows (T, K): the weight vector of each row."""
    D = Xs.shape[1]
    p = torch.tensor(params)
    t = 3
    l_F = p[t:t + D * S].reshape(D, S); t += D * S
    r_F = p[t:t + M * S].reshape(M, S); t += M * S
    F = l_F @ r_F.T
    l_P = p[t:t + S].reshape(1, S); t += S
    P = p[t:t + M].reshape(1, M)
    l_FC = l_P - l_F.mean(0)[None, :]
    FC = P - F.mean(0)[None, :]
    X = torch.tensor(Xs, requires_grad=True)
    FFs = torch.cat((X @ l_F + l_FC, X @ F + FC), 1)
    Phis = torch.exp(p[1]) * np.sqrt(2. / M) * torch.cat((torch.cos(FFs), torch.sin(FFs)), 1)
    f = (Phis * torch.tensor(Wrows)).sum(1)
    g, = torch.autograd.grad(f.sum(), X)                # rows are independent: the sum's gradient is the per-row one
    return f.detach().numpy(), g.numpy()


@pytest.mark.parametrize('D,S,M', CASES)
def test_closed_form_equals_autograd_of_the_literal_graph(D, S, M):
    params, alpha, Li, W, Xs, sidx = _problem(D, S, M, 11 + D)
    val, grad = R.sample_grad(Xs, W, sidx, params, S, M)
    f, g = _torch_literal(Xs, W.T[sidx], params, S, M)
    assert rel(val, f) < 1e-12 and rel(grad, g) < 1e-12
    # sidx = None means t % nsamp
    val2, grad2 = R.sample_grad(Xs, W, None, params, S, M)
    f2, g2 = _torch_literal(Xs, W.T[np.arange(Xs.shape[0]) % NSAMP], params, S, M)
    assert rel(val2, f2) < 1e-12 and rel(grad2, g2) < 1e-12


@pytest.mark.parametrize('D,S,M', CASES)
def test_closed_form_equals_finite_differences_of_the_sample_reference(D, S, M):
    seed = 29 + D
    params, alpha, Li, W, Xs, sidx = _problem(D, S, M, seed, T=12)
    val, grad = R.sample_grad(Xs, W, sidx, params, S, M)
    rows = np.arange(Xs.shape[0])
    f0 = SR.samples(Xs, alpha, Li, params, S, M, NSAMP, seed)[rows, sidx]
    assert rel(val, f0) < 1e-12
    h = 1e-5
    fd = np.empty_like(grad)
    for d in range(D):
        e = np.zeros(D); e[d] = h
        fp = SR.samples(Xs + e, alpha, Li, params, S, M, NSAMP, seed)[rows, sidx]
        fm = SR.samples(Xs - e, alpha, Li, params, S, M, NSAMP, seed)[rows, sidx]
        fd[:, d] = (fp - fm) / (2 * h)
    assert rel(grad, fd) < 1e-6


@pytest.mark.parametrize('D,S,M', CASES)
def test_weights_alpha_give_the_mean_and_its_gradient_exactly(D, S, M):
    params, alpha, Li, W, Xs, sidx = _problem(D, S, M, 5 + D)
    mu, _, dmu, _ = G.predict_grad(Xs, alpha, Li, params, S, M)
    val, grad = R.sample_grad(Xs, np.asarray(alpha).reshape(-1, 1), None, params, S, M)
    assert np.array_equal(grad, dmu)
    assert rel(val, mu.ravel()) < 1e-14
    # every column alpha: any sidx gives the same
    val3, grad3 = R.sample_grad(Xs, np.repeat(np.asarray(alpha).reshape(-1, 1), 3, 1), sidx % 3, params, S, M)
    assert np.array_equal(grad3, dmu) and np.array_equal(val3, val)


@pytest.mark.parametrize('mutation', ['swap_halves', 'drop_sign'])
def test_mutations_of_the_closed_form_fail_the_autograd_comparison(mutation):
    D, S, M = 5, 4, 60
    J = S + M
    params, alpha, Li, W, Xs, sidx = _problem(D, S, M, 16)
    _, g = _torch_literal(Xs, W.T[sidx], params, S, M)
    Phi = O.feature_map(Xs, params, D, S, M)
    pc, ps = Phi[:, :J], Phi[:, J:]
    Wr = W.T[sidx]
    wc, ws = Wr[:, :J], Wr[:, J:]
    Fa = G.fall(params, D, S, M)
    good = (pc * ws - ps * wc) @ Fa.T
    assert rel(good, g) < 1e-12
    bad = (pc * wc - ps * ws) @ Fa.T if mutation == 'swap_halves' else (pc * ws + ps * wc) @ Fa.T
    assert rel(bad, g) > 1e-2


def test_sample_grad_entry_point_declared_exported_and_checked_without_gpu():
    """scfgp_sample_grad is in the header, the library and the binding table, and refuses bad arguments before touching a device,
    leaving its outputs as they were."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'scfgp_hip.h')).read(), flags=re.S)
    assert re.search(r'\bscfgp_sample_grad\s*\(', header)
    assert 'scfgp_sample_grad' in _lib.SIGNATURES
    lib = _lib.load()
    fn = lib.scfgp_sample_grad
    assert fn.argtypes is not None and len(fn.argtypes) == 9
    D, S, M = 3, 2, 5
    K = 2 * (S + M)
    Xs = np.zeros((4, D)); W = np.zeros((K, 2))
    val = np.full(4, 7.5); grad = np.full((4, D), 7.5)
    p = _lib.dptr
    assert fn(None, p(Xs), 4, p(W), 2, None, 0, p(val), p(grad)) == -1
    ctx = ctypes.c_void_p()
    lib.scfgp_create(ctypes.byref(ctx), D, S, M, 0, 0, None)        # fails on a GPU-less box but hands back its context
    assert ctx.value
    try:
        for T in (0, -3):
            assert fn(ctx, p(Xs), T, p(W), 2, None, 0, p(val), p(grad)) == -1
        for mode in (-1, 3, 7):
            assert fn(ctx, p(Xs), 4, p(W), 2, None, mode, p(val), p(grad)) == -1
        assert b'bad arguments' in lib.scfgp_last_error(ctx)
        assert fn(ctx, None, 4, p(W), 2, None, 0, p(val), p(grad)) == -1
        assert fn(ctx, p(Xs), 4, None, 2, None, 0, p(val), p(grad)) == -1
        assert fn(ctx, p(Xs), 4, p(W), 2, None, 0, p(val), None) == -1          # grad is required
        for nsamp in (0, -1, 1025):
            assert fn(ctx, p(Xs), 4, p(W), nsamp, None, 0, p(val), p(grad)) == -1
            assert b'nsamp' in lib.scfgp_last_error(ctx)
        assert fn(ctx, p(Xs), 4, p(W), 2, None, 1, p(val), p(grad)) == -1       # no X scaler registered
        assert b'scaler' in lib.scfgp_last_error(ctx)
        assert fn(ctx, p(Xs), 4, p(W), 2, None, 0, p(val), p(grad)) == -1       # parameters not set
        assert b'parameters' in lib.scfgp_last_error(ctx)
        assert np.all(val == 7.5) and np.all(grad == 7.5)
    finally:
        lib.scfgp_destroy(ctx)
