"""CPU tier of scfgp_predict_grad: the closed-form input gradients of pred_func (tests/pred_grad_ref.py) against torch autograd of
the literal reference graph and against finite differences, the scalers' chain rules against finite differences of
scfgp_amd.scaler.Scaler, and the C entry point's argument checks (no GPU needed)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import scfgp_oracle as O
from scfgp_amd import _lib
from scfgp_amd.scaler import Scaler
from tests import pred_grad_ref as R

CASES = [(3, 1, 5), (5, 4, 60), (8, 2, 20), (4, 3, 17)]          # S = 1; K = 128; odd J


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def _problem(D, S, M, seed, N=150, T=40):
    rng = np.random.default_rng(seed)
    params = O.init_params(D, S, M, rng)
    params[:3] = (-1.0, 0.0, -1.0)
    X = rng.uniform(0, 1, (N, D))
    y = np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((N, 1))
    _, alpha, Li = O.forward(X, y, params, S, M, gauss_hermite=False)
    return params, alpha, Li, rng.uniform(0, 1, (T, D))


def _torch_literal(Xs, alpha, Li, params, S, M):
    """SCFGP/SCFGP.py:139-144 restated in torch float64; returns the autograd gradients of mu and std in Xs."""
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
    l_FFs = X @ l_F + l_FC
    FFs = torch.cat((l_FFs, X @ F + FC), 1)
    Phis = torch.cat((torch.cos(FFs), torch.sin(FFs)), 1)
    Phis = torch.exp(p[1]) * np.sqrt(2. / M) * Phis
    noise = torch.log(1 + torch.exp(p[2]))
    mu = Phis @ torch.tensor(alpha)
    std = (noise * (1 + ((Phis @ torch.tensor(Li).T) ** 2).sum(1))) ** 0.5
    gmu, = torch.autograd.grad(mu.sum(), X, retain_graph=True)      # rows are independent: the sum's gradient is the per-row one
    gsd, = torch.autograd.grad(std.sum(), X)
    return gmu.numpy(), gsd.numpy()


@pytest.mark.parametrize('D,S,M', CASES)
def test_closed_form_equals_autograd_of_the_literal_graph(D, S, M):
    params, alpha, Li, Xs = _problem(D, S, M, 11 + D)
    mu, sd, dmu, dsd = R.predict_grad(Xs, alpha, Li, params, S, M)
    mu0, sd0 = O.predict(Xs, alpha, Li, params, S, M)
    assert rel(mu, mu0) < 1e-13 and rel(sd, sd0) < 1e-13
    gmu, gsd = _torch_literal(Xs, alpha, Li, params, S, M)
    assert rel(dmu, gmu) < 1e-12 and rel(dsd, gsd) < 1e-12


@pytest.mark.parametrize('D,S,M', CASES)
def test_closed_form_equals_finite_differences_of_the_oracle(D, S, M):
    params, alpha, Li, Xs = _problem(D, S, M, 29 + D, T=12)
    _, _, dmu, dsd = R.predict_grad(Xs, alpha, Li, params, S, M)
    h = 1e-5
    fmu = np.empty_like(dmu); fsd = np.empty_like(dsd)
    for d in range(D):
        e = np.zeros(D); e[d] = h
        mp, sp = O.predict(Xs + e, alpha, Li, params, S, M)
        mm, sm = O.predict(Xs - e, alpha, Li, params, S, M)
        fmu[:, d] = (mp - mm).ravel() / (2 * h)
        fsd[:, d] = (sp - sm) / (2 * h)
    assert rel(dmu, fmu) < 1e-6 and rel(dsd, fsd) < 1e-6


def _x_data(rng, T=300, D=4):
    X = np.column_stack([rng.uniform(0.5, 3.0, T), rng.gamma(2.0, 1.0, T), rng.normal(1.0, 2.0, T), rng.uniform(-1, 1, T)])[:, :D]
    X[:, 0] = np.round(X[:, 0], 1)                   # few distinct values in one column (identity Box-Cox exponent)
    return np.column_stack([X[:, :2], np.full(T, 7.0), X[:, 2:]])        # one constant column: dropped by the scaler


@pytest.mark.parametrize('algo', Scaler.algos)
def test_x_scaler_jacobian_equals_finite_differences(algo):
    rng = np.random.default_rng(3)
    X = _x_data(rng)
    sc = Scaler(algo); sc.fit(X)
    assert 2 not in sc.data['cols']
    Xq = X[:20]
    J = R.x_scaler_deriv(sc, Xq)
    fd = np.empty_like(J)
    for k, c in enumerate(sc.data['cols']):
        h = 1e-6 * max(1.0, float(np.abs(X[:, c]).max()))
        Xp = Xq.copy(); Xp[:, c] += h
        Xm = Xq.copy(); Xm[:, c] -= h
        fd[:, k] = (sc.forward_transform(Xp)[:, k] - sc.forward_transform(Xm)[:, k]) / (2 * h)
    assert rel(J, fd) < 1e-6


@pytest.mark.parametrize('algo', Scaler.algos)
def test_y_back_transform_chain_equals_finite_differences(algo):
    rng = np.random.default_rng(4)
    y = rng.gamma(2.0, 1.0, (400, 1)) + 0.5
    sc = Scaler(algo); sc.fit(y)
    T = 16
    inv = algo.endswith('inv-normal')                 # backward takes the normal ppf: predictions live in (0, 1)
    mu = rng.uniform(0.3, 0.7, (T, 1)) if inv else rng.uniform(-1.0, 1.0, (T, 1))
    sd = rng.uniform(0.02, 0.08, T) if inv else rng.uniform(0.1, 0.4, T)
    dmu = rng.standard_normal((T, 3)); dsd = 0.1 * rng.standard_normal((T, 3))
    gmu, gsd = R.y_chain(sc, mu, sd, dmu, dsd)

    def band(h, k):                                   # mu_y, std_y along direction k of the inputs
        m = mu + h * dmu[:, k:k + 1]
        s = (sd + h * dsd[:, k])[:, None]
        return sc.backward_transform(m), 0.5 * (sc.backward_transform(m + s) - sc.backward_transform(m - s))

    h = 1e-6
    for k in range(3):
        (mp, sp), (mm, sm) = band(h, k), band(-h, k)
        assert rel(gmu[:, k], ((mp - mm) / (2 * h)).ravel()) < 1e-6
        assert rel(gsd[:, k], ((sp - sm) / (2 * h)).ravel()) < 1e-6


def test_predict_grad_entry_point_declared_exported_and_checked_without_gpu():
    """scfgp_predict_grad is in the header, the library and the binding table, and refuses bad arguments before touching a device."""
    import re, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'scfgp_hip.h')).read(), flags=re.S)
    assert re.search(r'\bscfgp_predict_grad\s*\(', header)
    assert 'scfgp_predict_grad' in _lib.SIGNATURES
    lib = _lib.load()
    fn = lib.scfgp_predict_grad
    assert fn.argtypes is not None and len(fn.argtypes) == 10
    D, S, M = 3, 2, 5
    K = 2 * (S + M)
    Xs = np.zeros((4, D)); alpha = np.zeros(K); Li = np.eye(K)
    mu = np.empty(4); sd = np.empty(4); dmu = np.empty((4, D)); dsd = np.empty((4, D))
    p = _lib.dptr
    assert fn(None, p(Xs), 4, p(alpha), p(Li), 0, p(mu), p(sd), p(dmu), p(dsd)) == -1
    ctx = ctypes.c_void_p()
    lib.scfgp_create(ctypes.byref(ctx), D, S, M, 0, 0, None)        # fails on a GPU-less box but hands back its context
    assert ctx.value
    try:
        assert fn(ctx, p(Xs), 0, p(alpha), p(Li), 0, p(mu), p(sd), p(dmu), p(dsd)) == -1
        assert fn(ctx, p(Xs), -3, p(alpha), p(Li), 0, p(mu), p(sd), p(dmu), p(dsd)) == -1
        for mode in (-1, 3, 7):
            assert fn(ctx, p(Xs), 4, p(alpha), p(Li), mode, p(mu), p(sd), p(dmu), p(dsd)) == -1
        assert b'bad arguments' in lib.scfgp_last_error(ctx)
        assert fn(ctx, p(Xs), 4, p(alpha), p(Li), 0, p(mu), p(sd), None, p(dsd)) == -1      # dmu is required
        assert fn(ctx, p(Xs), 4, p(alpha), p(Li), 1, p(mu), p(sd), p(dmu), p(dsd)) == -1      # no X scaler registered
        assert b'scaler' in lib.scfgp_last_error(ctx)
    finally:
        lib.scfgp_destroy(ctx)
